// w2xc_upconv_body.inc -- the body of upconv4x4_head (w2xc_upconv.hip; the design notes are there), included by the one-image kernel and by its batch form
// upconv4x4_head_batch.  The batch hooks, as in w2xc_last_body.inc:
//   UPB_ONLY(...)      the batch form's own statements (nothing in the one-image kernel)
//   UPB_SEL(b, s)      b in the batch form, s in the one-image kernel
//   UPB_IN / UPB_OUT   the input / output base of tile's image: d.in / d.out, or image `img`'s (+ img x bd.in_bs floats / + img x bd.out_bs floats, U8: bytes)
// Batch: bd.batch x ntiles tiles, image-major; a workgroup's run of consecutive tiles may straddle two images, so the image of a tile is derived per tile --
// in blk_load (the prefetch may already be the next image's) and for the stores -- and enters on the 64-bit bases only.
    constexpr int ROWS = 8, HW = 34, HH = ROWS + 2, NPIX = HH * HW;
    constexpr int NBLK = (NPIX + 15) / 16;
    constexpr int N = 16 * NOUT, NB16 = NOUT;
    constexpr int GS = N | 1;                  // odd LDS row stride
    constexpr int S4 = CIN / 16;
    extern __shared__ float lds[];
    float *G = lds;                            // [NBLK * 16][GS]
    float *Wl = lds + NBLK * 16 * GS;          // [S4 * 4][NB16][64]: the weight image as packed

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kk = lane >> 4, i = lane & 15;

    for (int e = threadIdx.x; e < S4 * 4 * NB16 * 64; e += 256) Wl[e] = d.wpk[e];
    float bo[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; o++) bo[o] = d.bias[o];
    __syncthreads();

    // the 16 channels-of-four of pixel block `blk` of tile `tile` (clamped: only pixels of the tile's overhang, which no kept output reads, ever clamp)
    auto blk_load = [&](int tile, int blk, f32x4 (&v)[S4]) {
        UPB_ONLY(const int img = tile / ntiles; tile -= img * ntiles;)   // (batch: the tile inside its image)
        const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
        int q = blk * 16 + i;
        q = q < NPIX ? q : NPIX - 1;
        const int py = q / HW, px = q - py * HW;
        const int gy = clampi(tile_y * ROWS + py + d.off_y, 0, d.in_h - 1);
        const int gx = clampi(tile_x * 32 + px + d.off_x, 0, d.in_w - 1);
        const f32x4 *src = reinterpret_cast<const f32x4 *>(UPB_IN + (long long)gy * d.in_rs + (long long)gx * CIN) + kk;
#pragma unroll
        for (int s4 = 0; s4 < S4; s4++) v[s4] = src[s4 * 4];
    };

    // this workgroup's run of consecutive tiles; runs that follow each other share an XCD (their tiles share halo pixels in its L2)
    const int ntot = UPB_SEL(bd.batch * ntiles, ntiles);   // tiles of the launch
    const int nwg = gridDim.x, per = (ntot + nwg - 1) / nwg;
    const int tile_first = xcd_remap(blockIdx.x, nwg) * per;
    const int tile_end = tile_first + per < ntot ? tile_first + per : ntot;
    f32x4 av[S4];
    if (tile_first < tile_end) blk_load(tile_first, wave, av);
    for (int gtile = tile_first; gtile < tile_end; gtile++) {   // (batch: a tile of the whole launch)
        UPB_ONLY(const int img = gtile / ntiles;)
        const int tile = UPB_SEL(gtile - img * ntiles, gtile);
        const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
        const int oy0 = tile_y * ROWS, ox0 = tile_x * 32;
        for (int blk = wave; blk < NBLK; blk += 4) {
            // the next block's loads (this tile's, or the first of the next tile) fly under this block's MFMAs
            f32x4 nv[S4];
            const bool more = blk + 4 < NBLK;
            const bool next_tile = !more && gtile + 1 < tile_end;
            if (more) blk_load(gtile, blk + 4, nv);
            else if (next_tile) blk_load(gtile + 1, wave, nv);   // (batch: the next tile's own image)
            f32x4 acc[NB16];
#pragma unroll
            for (int nb = 0; nb < NB16; nb++) acc[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s4 = 0; s4 < S4; s4++)
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int nb = 0; nb < NB16; nb++)
                        acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4][j], Wl[((s4 * 4 + j) * NB16 + nb) * 64 + lane], acc[nb], 0, 0, 0);
            // C/D map of the 16x16 MFMA: column = lane & 15 (n), row = 4 (lane >> 4) + r (pixel in block)
#pragma unroll
            for (int nb = 0; nb < NB16; nb++)
#pragma unroll
                for (int r = 0; r < 4; r++) G[(blk * 16 + kk * 4 + r) * GS + nb * 16 + i] = acc[nb][r];
            if (more || next_tile) {
#pragma unroll
                for (int s4 = 0; s4 < S4; s4++) av[s4] = nv[s4];
            }
        }
        __syncthreads();

        for (int p = threadIdx.x; p < 2 * ROWS * 64; p += 256) {
            const int yl = p >> 6, xl = p & 63;
            const int iy = yl >> 1, py = yl & 1, ix = xl >> 1, px = xl & 1;
            const int y = oy0 + iy, x = ox0 + ix;
            if (y >= d.out_h || x >= d.out_w) continue;
#pragma unroll
            for (int o = 0; o < NOUT; o++) {
                float v = 0.0f;
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int b = 0; b < 2; b++) {
                        const int r = 1 - py + 2 * a, s = 1 - px + 2 * b;
                        const int zy = iy + ((py + 3 - r) >> 1), zx = ix + ((px + 3 - s) >> 1);
                        v += G[(zy * HW + zx) * GS + (4 * r + s) * NOUT + o];
                    }
                v += bo[o];
                const long long at = (long long)o * d.out_cs + (long long)(2 * y + py) * d.out_rs + (long long)(2 * x + px) * d.out_ps;
                if constexpr (U8) reinterpret_cast<unsigned char *>(UPB_OUT)[at] = (unsigned char)clampi(__float2int_rn(v * 255.0f), 0, 255);
                else (UPB_OUT)[at] = v;
            }
        }
        __syncthreads();                                 // (G is rewritten by the next tile)
    }
