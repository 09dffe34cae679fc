// w2xc_rgb_to_yuv8_body.inc -- the body of k_rgb_to_yuv8 (w2xc_yuv_rgb.hip: centred chroma, the box mean) and of k_rgb_to_yuv8_sited (w2xc_yuv_rgb_sited.hip:
// chroma co-sited with luma along x and / or y, the 1-2-1 mean around luma 2k), included between the braces of a kernel with k_rgb_to_yuv8's parameters and
// template parameters and two constants in scope:
//   CX, CY   along x / y a chroma sample sits ON luma sample 2k
// The load of a thread's block, y', cb, cr of its pixels and the luma stores are the same for every siting.  Centred on both axes, a thread's chroma is the box mean
// of its own block and nothing is exchanged.  Co-sited (the exchange is written once for both widths: row_chroma, top_row_chroma, w2xc_yuv_tile.h):
//   x: the horizontal 1-2-1 of a luma row needs cb, cr of luma column 2 cx - 1, the RIGHT column of the left neighbour's block: one lane down in the wave's 32-lane
//      half.  Only lane 0 -- the tile's own left column -- converts that pixel from memory; at the plane's left edge the column clamps to the thread's own.
//   y: the vertical 1-2-1 needs the horizontal result of luma row 2 cy - 1, the BOTTOM row of the block one tile row up.  Every thread leaves the horizontal results
//      of its bottom rows in LDS (2 x YR_TCY x YR_TCX floats: 4 KB), a wave's half a run of 32 consecutive words; only tile row 0 -- ly = 0, the first of the two
//      blocks -- converts that luma row from memory, its left column exchanged as above; at the plane's top edge the row clamps to the block's own.
// A co-sited kernel keeps every thread in the loop (threads whose sample lies outside the plane work on the clamped sample and store nothing), so that the exchanges
// and the barriers are reached by all.  Stores stay the thread's own samples.
    constexpr int HX = SX ? 1 : 0, HY = SY ? 1 : 0;
    constexpr bool SITED = CX || CY;
    static_assert(!SITED || SX, "every layout with a subsampled axis subsamples x");
    static_assert(!CY || SY, "a co-sited y axis is a subsampled one");
    __shared__ float below[CY ? 2 * YR_TCY * YR_TCX : 1];   // CY: cb and cr of the horizontal pass of every block's bottom luma row
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const float cs = limited ? 224.0f : 255.0f;
    for (long long turn = blockIdx.x; turn < turns; turn += gridDim.x) {
        int cx0, cy0;
        const long long f = yuv_tile_at(turn, tiles, tiles_x, YR_TCX, YR_TCY, &cx0, &cy0);
        const float *s = rgb + f * is;
        unsigned char *oy = dy + f * yframe;
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
                unsigned char *d = oy + Y * yrow + X;
                const unsigned b0 = luma_u8(p[r][0].y, limited);
                if (SX && X + 1 < w) {
                    const unsigned b1 = luma_u8(p[r][HX].y, limited);
                    if (y16) *reinterpret_cast<unsigned short *>(d) = (unsigned short)(b0 | (b1 << 8));
                    else { d[0] = (unsigned char)b0; d[1] = (unsigned char)b1; }
                } else d[0] = (unsigned char)b0;
            }
            if (!SITED) {
                float cb, cr;
                chroma_mean<SX, SY>(p, &cb, &cr);
                const long long at = f * cframe + cy * crow + (long long)cx * dpx;
                du[at] = chroma_u8(cb, cs);
                dv[at] = chroma_u8(cr, cs);
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
                du[at] = chroma_u8(cb, cs);
                dv[at] = chroma_u8(cr, cs);
            }
        }
    }
