// w2xc_last_body.inc -- the body of conv3x3_last (w2xc_kernels.hip; the design notes are there), included by the one-image kernel and by its batch form
// conv3x3_last_batch (w2xc_conv_batch.hip); the batch hooks FLB_ONLY / FLB_SEL / FLB_IN / FLB_OUT are those of w2xc_first_body.inc.  Batch: bd.batch x ntiles
// tiles, image-major; the image of a tile is derived per tile, in blk_load (the prefetch may already be the next image's) and for the stores.
    constexpr int ROWS = 8, HW = 34, HH = ROWS + 2, NPIX = HH * HW;
    constexpr int NBLK = (NPIX + 15) / 16;
    constexpr int N = 9 * COUT, NB16 = (N + 15) / 16;
    constexpr int GS = N | 1;                  // odd LDS row stride
    constexpr int S4 = CIN / 16;
    __shared__ float G[NBLK * 16 * GS];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kk = lane >> 4, i = lane & 15;

    // the layer's weights once per workgroup, which walks LAST_TPW consecutive tiles (round 6: one tile per workgroup re-read the 16 KiB image per tile,
    // and a wave's pixel blocks ran load -> wait -> 64 MFMAs one after the other: 3.9 TB/s of reads on 128 -> 3)
    float b[S4][4][NB16];
#pragma unroll
    for (int s4 = 0; s4 < S4; s4++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int nb = 0; nb < NB16; nb++) b[s4][j][nb] = d.wpk[((s4 * 4 + j) * NB16 + nb) * 64 + lane];

    // the 16 channels-of-four of pixel block `blk` of tile `tile` (clamped: the haloed tile's pixels outside the plane repeat the edge)
    auto blk_load = [&](int tile, int blk, f32x4 (&v)[S4]) {
        FLB_ONLY(const int img = tile / ntiles; tile -= img * ntiles;)   // (batch: the tile inside its image)
        const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
        int q = blk * 16 + i;
        q = q < NPIX ? q : NPIX - 1;
        const int py = q / HW, px = q - py * HW;
        const int gy = clampi(tile_y * ROWS + py + d.off_y, 0, d.in_h - 1);
        const int gx = clampi(tile_x * 32 + px + d.off_x, 0, d.in_w - 1);
        const f32x4 *src = reinterpret_cast<const f32x4 *>(FLB_IN + (long long)gy * d.in_rs + (long long)gx * CIN) + kk;
#pragma unroll
        for (int s4 = 0; s4 < S4; s4++) v[s4] = src[s4 * 4];
    };

    float bo[COUT];
#pragma unroll
    for (int o = 0; o < COUT; o++) bo[o] = d.bias[o];
    const int ntot = FLB_SEL(bd.batch * ntiles, ntiles);   // tiles of the launch
    const int tile_base = xcd_remap(blockIdx.x, (ntot + LAST_TPW - 1) / LAST_TPW) * LAST_TPW;
    f32x4 av[S4];
    if (tile_base < ntot) blk_load(tile_base, wave, av);
    // (register VALUES from here on: left pending, the weights' waits sit INSIDE the loop -- s_waitcnt vmcnt(7) behind the eight loads of the next
    //  block, i.e. a wait for the first of those -- in every pass)
#pragma unroll
    for (int s4 = 0; s4 < S4; s4++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int nb = 0; nb < NB16; nb++) asm volatile("" : "+v"(b[s4][j][nb]));
    for (int it = 0; it < LAST_TPW; it++) {
        const int gtile = tile_base + it;                // (batch: a tile of the whole launch)
        if (gtile >= ntot) break;                        // (workgroup-uniform)
        FLB_ONLY(const int img = gtile / ntiles;)
        const int tile = FLB_SEL(gtile - img * ntiles, gtile);
        const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
        const int oy0 = tile_y * ROWS, ox0 = tile_x * 32;
        for (int blk = wave; blk < NBLK; blk += 4) {
            // the next block's loads (this tile's, or the first of the next tile) fly under this block's MFMAs
            f32x4 nv[S4];
            const bool more = blk + 4 < NBLK;
            const bool next_tile = !more && it + 1 < LAST_TPW && gtile + 1 < ntot;
            if (more) blk_load(gtile, blk + 4, nv);
            else if (next_tile) blk_load(gtile + 1, wave, nv);
            f32x4 acc[NB16];
#pragma unroll
            for (int nb = 0; nb < NB16; nb++) acc[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s4 = 0; s4 < S4; s4++)
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int nb = 0; nb < NB16; nb++)
                        acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4][j], b[s4][j][nb], acc[nb], 0, 0, 0);
            // C/D map of 16x16 MFMA: column = lane&15 (n), row = 4*(lane>>4) + r (pixel in block)
#pragma unroll
            for (int nb = 0; nb < NB16; nb++) {
                const int n = nb * 16 + i;
                if (n < N) {
#pragma unroll
                    for (int r = 0; r < 4; r++) G[(blk * 16 + kk * 4 + r) * GS + n] = acc[nb][r];
                }
            }
            if (more || next_tile) {
#pragma unroll
                for (int s4 = 0; s4 < S4; s4++) av[s4] = nv[s4];
            }
        }
        __syncthreads();

        for (int p = threadIdx.x; p < ROWS * 32; p += 256) {
            const int py = p >> 5, px = p & 31;
            const int y = oy0 + py, x = ox0 + px;
            if (y >= d.out_h || x >= d.out_w) continue;
#pragma unroll
            for (int o = 0; o < COUT; o++) {
                float v = 0.0f;
#pragma unroll
                for (int tap = 0; tap < 9; tap++)
                    v += G[((py + tap / 3) * HW + px + tap % 3) * GS + tap * COUT + o];
                const long long at = (long long)o * d.out_cs + (long long)y * d.out_rs + (long long)x * d.out_ps;
                if constexpr (U8) reinterpret_cast<unsigned char *>(FLB_OUT)[at] = (unsigned char)clampi(__float2int_rn(leaky(v + bo[o]) * 255.0f), 0, 255);
                else (FLB_OUT)[at] = leaky(v + bo[o]);
            }
        }
        __syncthreads();                                 // (G is rewritten by the next tile)
    }
