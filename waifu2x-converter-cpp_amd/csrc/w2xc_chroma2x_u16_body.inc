// w2xc_chroma2x_u16_body.inc -- the body of k_chroma2x_u16 (w2xc_yuv16.hip: centred chroma) and of k_chroma2x_u16_sited (w2xc_yuv16_sited.hip: chroma co-sited
// with luma along x and / or y), included between the braces of a kernel with k_chroma2x_u16's parameters, the template parameter LOAD and two constants in scope:
//   CX, CY   along x / y a chroma sample sits ON luma sample 2k: the quad's two outputs lie at t = 0.375 and 0.875 of their source pixel instead of 0.25 and 0.75
// Nothing else depends on them: not the quads, the halo, the loaders, the crop or the stores (the comment at k_chroma2x_u16 describes all of these).
    __shared__ float tile[2][CH_SH * CH_LD];
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    float cxa[4], cxb[4], cya[4], cyb[4];   // the coefficients of a quad's first and second column, first and second row
    cubic_coeffs(CX ? 0.375f : 0.25f, cxa);
    cubic_coeffs(CX ? 0.875f : 0.75f, cxb);
    cubic_coeffs(CY ? 0.375f : 0.25f, cya);
    cubic_coeffs(CY ? 0.875f : 0.75f, cyb);
    for (long long turn = blockIdx.x; turn < turns; turn += gridDim.x) {   // a turn: one tile of the planes of one frame
        const long long f = turn / tiles, t = turn - f * tiles;
        const int qy0 = (int)(t / tiles_x) * CH_TQY, qx0 = (int)(t % tiles_x) * CH_TQX;
        const int gx0 = qx0 - 2, gy0 = qy0 - 2;   // the source pixel of LDS word (0, 0)
        __syncthreads();   // (the tiles of the loop's previous turn have been read)
        if (LOAD == 2) {
            const unsigned short *s = su + f * sframe;
            for (int i = threadIdx.x; i < CH_SH * CH_SW; i += 256) {
                const int r = i / CH_SW, c = i - r * CH_SW;
                const unsigned w2 = *reinterpret_cast<const unsigned *>(s + clampi(gy0 + r, 0, ch - 1) * srow + (long long)clampi(gx0 + c, 0, cw - 1) * 2);
                tile[0][r * CH_LD + c] = (float)u16_value(w2 & 0xFFFFu, rshift, max) * inv_max;
                tile[1][r * CH_LD + c] = (float)u16_value(w2 >> 16, rshift, max) * inv_max;
            }
        } else {
            for (int v = 0; v < npl; v++) {
                const unsigned short *s = (v ? sv : su) + f * sframe;
                float *T = tile[v];
                if (LOAD == 1) {
                    // column groups of four source pixels from gx0 - 2 (a multiple of 4) on: ten cover the CH_SW columns
                    for (int i = threadIdx.x; i < CH_SH * 10; i += 256) {
                        const int r = i / 10, g = i - r * 10;
                        const int gx4 = gx0 - 2 + 4 * g;
                        const unsigned short *row = s + clampi(gy0 + r, 0, ch - 1) * srow;
                        unsigned b[4];
                        if (gx4 >= 0 && gx4 + 3 < cw) {
                            const uint2 w4 = *reinterpret_cast<const uint2 *>(row + gx4);
                            b[0] = w4.x & 0xFFFFu; b[1] = w4.x >> 16; b[2] = w4.y & 0xFFFFu; b[3] = w4.y >> 16;
                        } else {
#pragma unroll
                            for (int k = 0; k < 4; k++) b[k] = row[clampi(gx4 + k, 0, cw - 1)];
                        }
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const int c = 4 * g - 2 + k;
                            if (c >= 0 && c < CH_SW) T[r * CH_LD + c] = (float)u16_value(b[k], rshift, max) * inv_max;
                        }
                    }
                } else {
                    for (int i = threadIdx.x; i < CH_SH * CH_SW; i += 256) {
                        const int r = i / CH_SW, c = i - r * CH_SW;
                        T[r * CH_LD + c] = (float)u16_value(s[clampi(gy0 + r, 0, ch - 1) * srow + (long long)clampi(gx0 + c, 0, cw - 1) * spx], rshift, max) * inv_max;
                    }
                }
            }
        }
        __syncthreads();
        const int qx = qx0 + lx, X0 = 2 * qx - 1;   // the quad's columns X0 (centred: t = 0.25) and X0 + 1 (t = 0.75)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int qr = ly + j * (CH_TQY / 2), Y0 = 2 * (qy0 + qr) - 1;   // rows Y0 (t = 0.25) and Y0 + 1 (t = 0.75)
            if (X0 >= ow || Y0 >= oh) continue;
            unsigned o[2][4] = {};   // per plane: (Y0, X0), (Y0, X0 + 1), (Y0 + 1, X0), (Y0 + 1, X0 + 1), packed words
#pragma unroll
            for (int v = 0; v < 2; v++) {
                if (v >= npl) continue;
                float ra[4], rb[4];   // the horizontal pass of the four rows, for either column
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float *S = tile[v] + (qr + k) * CH_LD + lx;
                    ra[k] = chroma_row_sum(S, cxa);
                    rb[k] = chroma_row_sum(S, cxb);
                }
                o[v][0] = to_u16(chroma_row_sum(ra, cya), fmax, max) << lshift;
                o[v][1] = to_u16(chroma_row_sum(rb, cya), fmax, max) << lshift;
                o[v][2] = to_u16(chroma_row_sum(ra, cyb), fmax, max) << lshift;
                o[v][3] = to_u16(chroma_row_sum(rb, cyb), fmax, max) << lshift;
            }
            const long long at = f * dframe + Y0 * drow + (long long)X0 * dpx;
            const bool ok[4] = {Y0 >= 0 && X0 >= 0, Y0 >= 0 && X0 + 1 < ow, Y0 + 1 < oh && X0 >= 0, Y0 + 1 < oh && X0 + 1 < ow};
            const long long off[4] = {0, dpx, drow, drow + dpx};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!ok[k]) continue;
                if (pair) *reinterpret_cast<unsigned *>(du + at + off[k]) = o[0][k] | (o[1][k] << 16);
                else {
                    du[at + off[k]] = (unsigned short)o[0][k];
                    if (npl == 2) dv[at + off[k]] = (unsigned short)o[1][k];
                }
            }
        }
    }
