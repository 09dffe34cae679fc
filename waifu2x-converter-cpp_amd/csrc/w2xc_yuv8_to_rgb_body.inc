// w2xc_yuv8_to_rgb_body.inc -- the body of k_yuv8_to_rgb (w2xc_yuv_rgb.hip: centred chroma) and of k_yuv8_to_rgb_sited (w2xc_yuv_rgb_sited.hip: chroma co-sited with luma along x and / or y), included between the
// braces of a kernel with k_yuv8_to_rgb's parameters and template parameters and two constants in scope:
//   CX, CY   along x / y a chroma sample sits ON luma sample 2k: chroma at luma 2k is C[k], at 2k + 1 it is 0.5 C[k] + 0.5 C[k + 1] (chroma_at_luma_sited)
// Nothing else depends on them: the tiles, their halo, the loaders and the stores are those the comment at k_yuv8_to_rgb describes.
    constexpr int HX = SX ? 1 : 0, HY = SY ? 1 : 0;          // the halo
    constexpr int SW = YR_TCX + 2 * HX, SH = YR_TCY + 2 * HY;   // the chroma tile in LDS
    constexpr int LW = YR_TCX << HX, LH = YR_TCY << HY;       // the luma tile
    __shared__ float ctile[2][(YR_TCY + 2) * YR_LD];
    __shared__ __attribute__((aligned(4))) unsigned char ytile[2 * YR_TCY * YR_YLD];
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const float ky = limited ? (float)(1.0 / 219.0) : (float)(1.0 / 255.0), kc = limited ? (float)(1.0 / 224.0) : (float)(1.0 / 255.0);
    const float y0 = limited ? 16.0f : 0.0f;
    for (long long turn = blockIdx.x; turn < turns; turn += gridDim.x) {   // a turn: one tile of one frame
        int cx0, cy0;
        const long long f = yuv_tile_at(turn, tiles, tiles_x, YR_TCX, YR_TCY, &cx0, &cy0);
        const int X0 = cx0 << HX, Y0 = cy0 << HY;   // the tile's first luma sample
        const unsigned char *fy = sy + f * yframe;
        __syncthreads();   // (the tiles of the loop's previous turn have been read)
#pragma unroll
        for (int v = 0; v < 2; v++) {
            const unsigned char *s = (v ? sv : su) + f * cframe;
            float *tile = ctile[v];
            if (DW && spx == 1) {
                // column groups of four samples from cx0 - 4 HX (a multiple of 4) on
                constexpr int NG = YR_TCX / 4 + 2 * HX;
                for (int i = threadIdx.x; i < SH * NG; i += 256) {
                    const int r = i / NG, g = i - r * NG;
                    const int gx4 = cx0 - 4 * HX + 4 * g;
                    const unsigned char *row = s + clampi(cy0 - HY + r, 0, ch - 1) * crow;
                    unsigned b[4];
                    if (gx4 >= 0 && gx4 + 3 < cw) {
                        const unsigned w4 = *reinterpret_cast<const unsigned *>(row + gx4);
                        b[0] = w4 & 255u; b[1] = (w4 >> 8) & 255u; b[2] = (w4 >> 16) & 255u; b[3] = w4 >> 24;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; k++) b[k] = row[clampi(gx4 + k, 0, cw - 1)];
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int c = 4 * g - 3 * HX + k;
                        if (c >= 0 && c < SW) tile[r * YR_LD + c] = (float)b[k];
                    }
                }
            } else {
                for (int i = threadIdx.x; i < SH * SW; i += 256) {
                    const int r = i / SW, c = i - r * SW;
                    tile[r * YR_LD + c] = (float)s[clampi(cy0 - HY + r, 0, ch - 1) * crow + (long long)clampi(cx0 - HX + c, 0, cw - 1) * spx];
                }
            }
        }
        // luma: rows Y0 .. Y0 + LH - 1, columns X0 .. X0 + LW - 1 where they lie in the plane (nothing else of the tile is read below)
        if (DW) {
            constexpr int NG = LW / 4;
            for (int i = threadIdx.x; i < LH * NG; i += 256) {
                const int r = i / NG, g = i - r * NG;
                const int x4 = X0 + 4 * g;
                if (Y0 + r >= h || x4 >= w) continue;
                const unsigned char *row = fy + (Y0 + r) * yrow;
                unsigned w4;
                if (x4 + 3 < w) w4 = *reinterpret_cast<const unsigned *>(row + x4);
                else {
                    w4 = row[x4];
                    if (x4 + 1 < w) w4 |= (unsigned)row[x4 + 1] << 8;
                    if (x4 + 2 < w) w4 |= (unsigned)row[x4 + 2] << 16;
                }
                *reinterpret_cast<unsigned *>(ytile + r * YR_YLD + 4 * g) = w4;
            }
        } else {
            for (int i = threadIdx.x; i < LH * LW; i += 256) {
                const int r = i / LW, c = i - r * LW;
                if (Y0 + r < h && X0 + c < w) ytile[r * YR_YLD + c] = fy[(Y0 + r) * yrow + X0 + c];
            }
        }
        __syncthreads();
        float *o = rgb + f * is;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int tr = ly + j * (YR_TCY / 2), cx = cx0 + lx, cy = cy0 + tr;
            if (cx >= cw || cy >= ch) continue;
            float cu[2][1 + HY][1 + HX];   // U and V at the block's luma samples, from the thread's own sample
#pragma unroll
            for (int v = 0; v < 2; v++) chroma_at_luma_sited<SX, SY, CX, CY>(ctile[v] + (tr + HY) * YR_LD + lx + HX, YR_LD, cu[v]);
#pragma unroll
            for (int r = 0; r < 1 + HY; r++) {
                const int Y = (cy << HY) + r;
                if (Y >= h) continue;
                float px[3][1 + HX];   // R, G, B of the row's pixels
#pragma unroll
                for (int q = 0; q < 1 + HX; q++) {
                    const float y = ((float)ytile[((tr << HY) + r) * YR_YLD + (lx << HX) + q] - y0) * ky;
                    rgb_px(m, y, (cu[0][r][q] - 128.0f) * kc, (cu[1][r][q] - 128.0f) * kc, px, q);
                }
                const int X = cx << HX;
                float *d = o + (long long)Y * w + X;
                if (SX && v2) {   // (w is even: the second pixel lies in the row)
#pragma unroll
                    for (int p = 0; p < 3; p++) *reinterpret_cast<float2 *>(d + p * ps) = make_float2(px[p][0], px[p][HX]);
                } else {
#pragma unroll
                    for (int p = 0; p < 3; p++) {
                        d[p * ps] = px[p][0];
                        if (SX && X + 1 < w) d[p * ps + 1] = px[p][HX];
                    }
                }
            }
        }
    }
