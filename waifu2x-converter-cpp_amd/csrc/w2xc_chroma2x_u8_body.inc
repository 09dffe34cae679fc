// w2xc_chroma2x_u8_body.inc -- the body of k_chroma2x_u8 (w2xc_yuv.hip: centred chroma) and of k_chroma2x_u8_sited (w2xc_yuv_sited.hip: chroma co-sited with
// luma along x and / or y), included between the braces of a kernel with k_chroma2x_u8's parameters, the template parameter DW and two constants in scope:
//   CX, CY   along x / y a chroma sample sits ON luma sample 2k: the quad's two outputs lie at t = 0.375 and 0.875 of their source pixel instead of 0.25 and 0.75
// Nothing else depends on them: not the quads, the halo, the loaders, the crop or the stores (the comment at k_chroma2x_u8 describes all of these).
    __shared__ float tile[CH_SH * CH_LD];
    const float s255 = (float)(1.0 / 255.0);
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    float cxa[4], cxb[4], cya[4], cyb[4];   // the coefficients of a quad's first and second column, first and second row
    cubic_coeffs(CX ? 0.375f : 0.25f, cxa);
    cubic_coeffs(CX ? 0.875f : 0.75f, cxb);
    cubic_coeffs(CY ? 0.375f : 0.25f, cya);
    cubic_coeffs(CY ? 0.875f : 0.75f, cyb);
    for (long long turn = blockIdx.x; turn < turns; turn += gridDim.x) {   // a turn: one tile of one plane of one frame
        const long long p = turn / tiles, t = turn - p * tiles;
        const long long f = p / npl;
        const int v = (int)(p - f * npl);
        const unsigned char *s = (v ? sv : su) + f * sframe;
        unsigned char *d = (v ? dv : du) + f * dframe;
        const int qy0 = (int)(t / tiles_x) * CH_TQY, qx0 = (int)(t % tiles_x) * CH_TQX;
        const int gx0 = qx0 - 2, gy0 = qy0 - 2;   // the source pixel of LDS word (0, 0)
        __syncthreads();   // (the tile of the loop's previous turn has been read)
        if (DW) {
            // column groups of four source pixels from gx0 - 2 (a multiple of 4) on: ten cover the CH_SW columns
            for (int i = threadIdx.x; i < CH_SH * 10; i += 256) {
                const int r = i / 10, g = i - r * 10;
                const int gx4 = gx0 - 2 + 4 * g;
                const unsigned char *row = s + clampi(gy0 + r, 0, ch - 1) * srow;
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
                    const int c = 4 * g - 2 + k;
                    if (c >= 0 && c < CH_SW) tile[r * CH_LD + c] = (float)b[k] * s255;
                }
            }
        } else {
            for (int i = threadIdx.x; i < CH_SH * CH_SW; i += 256) {
                const int r = i / CH_SW, c = i - r * CH_SW;
                tile[r * CH_LD + c] = (float)s[clampi(gy0 + r, 0, ch - 1) * srow + (long long)clampi(gx0 + c, 0, cw - 1) * spx] * s255;
            }
        }
        __syncthreads();
        const int qx = qx0 + lx, X0 = 2 * qx - 1;   // the quad's columns X0 (centred: t = 0.25) and X0 + 1 (t = 0.75)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int qr = ly + j * (CH_TQY / 2), Y0 = 2 * (qy0 + qr) - 1;   // rows Y0 (t = 0.25) and Y0 + 1 (t = 0.75)
            if (X0 >= ow || Y0 >= oh) continue;
            float ra[4], rb[4];   // the horizontal pass of the four rows, for either column
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float *S = tile + (qr + k) * CH_LD + lx;
                ra[k] = chroma_row_sum(S, cxa);
                rb[k] = chroma_row_sum(S, cxb);
            }
            unsigned char *o = d + Y0 * drow + (long long)X0 * dpx;
            const bool left = X0 >= 0, right = X0 + 1 < ow;
            if (Y0 >= 0) {
                if (left) o[0] = to_u8(chroma_row_sum(ra, cya));
                if (right) o[dpx] = to_u8(chroma_row_sum(rb, cya));
            }
            if (Y0 + 1 < oh) {
                if (left) o[drow] = to_u8(chroma_row_sum(ra, cyb));
                if (right) o[drow + dpx] = to_u8(chroma_row_sum(rb, cyb));
            }
        }
    }
