// w2xc_rgb_to_yuv16_body.inc -- the body of k_rgb_to_yuv16 (w2xc_yuv16_rgb.hip: centred chroma, the box mean) and of k_rgb_to_yuv16_sited
// (w2xc_yuv16_rgb_sited.hip: chroma co-sited with luma along x and / or y, the 1-2-1 mean around luma 2k), included between the braces of a kernel with
// k_rgb_to_yuv16's parameters and template parameters and two constants in scope:
//   CX, CY   along x / y a chroma sample sits ON luma sample 2k
// The structure is w2xc_rgb_to_yuv8_body.inc's, which describes the two exchanges (a lane for column 2 cx - 1, 4 KB of LDS for luma row 2 cy - 1; row_chroma and
// top_row_chroma, w2xc_yuv_tile.h, are the same code for both widths); what differs is the roundings and the stores, those of k_rgb_to_yuv16.
    constexpr int HX = SX ? 1 : 0, HY = SY ? 1 : 0;
    constexpr bool SITED = CX || CY;
    static_assert(!SITED || SX, "every layout with a subsampled axis subsamples x");
    static_assert(!CY || SY, "a co-sited y axis is a subsampled one");
    __shared__ float below[CY ? 2 * YR_TCY * YR_TCX : 1];   // CY: cb and cr of the horizontal pass of every block's bottom luma row
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    // The co-sited forms hold more uniform values at once than there are scalar registers (the top-left form kept three in lanes of a vector register): the four
    // rounding constants, operands of vector arithmetic alone, live in vector registers there instead.  The centred kernel's code is what it was.
    float ysv = ys, y0v = y0, csv = cs, c0v = c0;
    if (SITED) asm volatile("" : "+v"(ysv), "+v"(y0v), "+v"(csv), "+v"(c0v));
    for (long long turn = blockIdx.x; turn < turns; turn += gridDim.x) {
        int cx0, cy0;
        const long long f = yuv_tile_at(turn, tiles, tiles_x, YR_TCX, YR_TCY, &cx0, &cy0);
        const float *s = rgb + f * is;
        unsigned short *oy = dy + f * yframe;
        float hb[2][1 + HY], hr[2][1 + HY];   // co-sited: cb and cr of the horizontal pass of the rows of the thread's two blocks
        float tb = 0.0f, tr_ = 0.0f;           // ... and, in tile row 0, of the luma row above the tile
        if (CY) __syncthreads();   // (the rows of the loop's previous turn have been read)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int cx = cx0 + lx, cy = cy0 + ly + j * (YR_TCY / 2);
            const bool in = cx < cw && cy < ch;
            if (!SITED && !in) continue;
            const int bx = SITED ? min(cx, cw - 1) : cx, by = SITED ? min(cy, ch - 1) : cy;   // the block that is loaded
            YCC p[1 + HY][1 + HX];
#pragma unroll
            for (int r = 0; r < 1 + HY; r++) {
                const int Y = min((by << HY) + r, h - 1);
                if (SX && v2) {   // (w is even: no block is cut at the right edge)
                    const float *e = s + (long long)Y * w + (bx << HX);
                    const float2 R = *reinterpret_cast<const float2 *>(e), G = *reinterpret_cast<const float2 *>(e + ps), B = *reinterpret_cast<const float2 *>(e + 2 * ps);
                    p[r][0] = to_ycc(m, R.x, G.x, B.x);
                    p[r][HX] = to_ycc(m, R.y, G.y, B.y);
                    continue;
                }
#pragma unroll
                for (int q = 0; q < 1 + HX; q++) {
                    const int X = min((bx << HX) + q, w - 1);
                    const float *e = s + (long long)Y * w + X;
                    p[r][q] = to_ycc(m, e[0], e[ps], e[2 * ps]);
                }
            }
#pragma unroll
            for (int r = 0; r < 1 + HY; r++) {
                const int Y = (cy << HY) + r, X = cx << HX;
                if (Y >= h || (SITED && !in)) continue;
                unsigned short *d = oy + Y * yrow + X;
                const unsigned b0 = luma_u16(p[r][0].y, limited, ysv, y0v, max) << yshift;
                if (SX && X + 1 < w) {
                    const unsigned b1 = luma_u16(p[r][HX].y, limited, ysv, y0v, max) << yshift;
                    if (y32) *reinterpret_cast<unsigned *>(d) = b0 | (b1 << 16);
                    else { d[0] = (unsigned short)b0; d[1] = (unsigned short)b1; }
                } else d[0] = (unsigned short)b0;
            }
            if (!SITED) {
                float cb, cr;
                chroma_mean<SX, SY>(p, &cb, &cr);
                const long long at = f * cframe + cy * crow + (long long)cx * dpx;
                const unsigned U = to_u16(cb, csv, c0v, max) << cshift, V = to_u16(cr, csv, c0v, max) << cshift;
                if (uv32) *reinterpret_cast<unsigned *>(du + at) = U | (V << 16);
                else {
                    du[at] = (unsigned short)U;
                    dv[at] = (unsigned short)V;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 1 + HY; r++)
                    row_chroma<CX>(m, s, ps, w, min((by << HY) + r, h - 1), cx0, lx, p[r][0], p[r][HX], &hb[j][r], &hr[j][r]);
                if (CY) {
                    const int tr = ly + j * (YR_TCY / 2);
                    below[tr * YR_TCX + lx] = hb[j][HY];
                    below[(YR_TCY + tr) * YR_TCX + lx] = hr[j][HY];
                    if (j == 0 && ly == 0) top_row_chroma<CX>(m, s, ps, w, cx0, cy0, bx, lx, hb[0][0], hr[0][0], &tb, &tr_);
                }
            }
        }
        if (SITED) {
            if (CY) __syncthreads();
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int tr = ly + j * (YR_TCY / 2), cx = cx0 + lx, cy = cy0 + tr;
                float cb, cr;
                if (CY) {
                    const int up = tr ? tr - 1 : 0;   // (tile row 0 reads a word of its own and drops it)
                    const float ab = tr ? below[up * YR_TCX + lx] : tb, ar = tr ? below[(YR_TCY + up) * YR_TCX + lx] : tr_;
                    cb = mean121(ab, hb[j][0], hb[j][HY]);
                    cr = mean121(ar, hr[j][0], hr[j][HY]);
                } else if (SY) {
                    cb = (hb[j][0] + hb[j][HY]) * 0.5f;
                    cr = (hr[j][0] + hr[j][HY]) * 0.5f;
                } else { cb = hb[j][0]; cr = hr[j][0]; }
                if (cx >= cw || cy >= ch) continue;
                const long long at = f * cframe + cy * crow + (long long)cx * dpx;
                const unsigned U = to_u16(cb, csv, c0v, max) << cshift, V = to_u16(cr, csv, c0v, max) << cshift;
                if (uv32) *reinterpret_cast<unsigned *>(du + at) = U | (V << 16);
                else {
                    du[at] = (unsigned short)U;
                    dv[at] = (unsigned short)V;
                }
            }
        }
    }
