// w2xc_kernels.hip -- gfx950 (MI355X, CDNA4) kernels for the waifu2x 3x3-conv + bias + LeakyReLU
// layer, i.e. the body of Model::filterWorker (/root/reference/src/modelHandler.cpp:117-159).
//
// Four kernels, one launch per layer per band (see w2xc_kernels.h for the addressing contract):
//
//   conv3x3_direct      any (cin, cout), any strides.  VALU, one thread per output pixel and 8
//                       output planes; sums in the REFERENCE'S order with unfused mul/add, so it
//                       is bit-exact against the CPU oracle.  Fallback + on-GPU cross-check.
//   conv3x3_mfma2       cin, cout in {32,64,128}.  NHWC fp32 activations; persistent workgroups (one per CU); the
//                       10 x 34 pixel halo tile of a 32-channel slice and the weights of one (slice, tap) stage reach
//                       LDS by LDS-DMA (XOR-swizzled: conflict-free ds_read_b128), the 3x3xCinxCout contraction is an
//                       implicit GEMM on v_mfma_f32_32x32x2_f32 (M = 32 pixels of one row, N = 32 output planes,
//                       K = (tap, cin)), bias + LeakyReLU fused into the epilogue, NHWC stores in 128-byte runs.
//                       (The first-generation kernel it replaced -- register-staged tiles, weights from L2 -- was
//                       removed in round 2; its history is in DESIGN.md 3.)
//   conv3x3_first       cin <= 3 (layer 1): planar input, clamp-to-edge folded into the LDS fill
//                       (this is cv::copyMakeBorder, convertRoutine.cpp:35), K = 9*cin on the same
//                       32x32x2 MFMA, NHWC output.  HBM-write bound.
//   conv3x3_last        cout <= 3 (layer 7): "taps as N": G[q][tap,o] = sum_c in[q][c]*W[o][c][tap]
//                       for every haloed pixel q on v_mfma_f32_16x16x4_f32 straight from global
//                       memory, then out[p][o] = sum_tap G[p+tap][tap,o] through LDS; planar
//                       output written at its final place (the crop/stitch of
//                       convertRoutine.cpp:40-46,143-161).  HBM-read bound.
//
// fp32 MFMA on gfx950 is an exact k-ordered fmaf chain at the f32 vector rate (157.3 TF peak).
// Kernels and launchers only: w2xc_pick_kernel and the weight images (w2xc_pack_weights) are in w2xc_pack.cpp.
#include "w2xc_kernels.h"
#include "w2xc_device.h"
#include "w2xc_launch.hpp"
#include "w2xc_layout.h"

// ------------------------------------------------------------------------------------------------
// conv3x3_direct: reference-ordered VALU kernel (bit-exact vs the oracle).
//   weights packed [cin][9][cout8-padded]: for one (i, tap) the 8 output planes of a group are
//   contiguous and wave-uniform -> scalar loads.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) conv3x3_direct(W2xcConvDesc d, int cout_pad)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    const int og = blockIdx.z * DIRECT_CG;
    if (x >= d.out_w || y >= d.out_h) return;
    long long roff[3], coff[3];
#pragma unroll
    for (int r = 0; r < 3; r++) roff[r] = (long long)(clampi(y + r + d.off_y, 0, d.in_h - 1) >> d.in_shift) * d.in_rs;
#pragma unroll
    for (int c = 0; c < 3; c++) coff[c] = (long long)(clampi(x + c + d.off_x, 0, d.in_w - 1) >> d.in_shift) * d.in_ps;
    float acc[DIRECT_CG];
#pragma unroll
    for (int k = 0; k < DIRECT_CG; k++) acc[k] = 0.0f;                                  // :131-132
    for (int i = 0; i < d.cin; i++) {                                                   // :134
        const float *ip = d.in + (long long)i * d.in_cs;
        float v[9];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) v[r * 3 + c] = ip[roff[r] + coff[c]];
        const float *wp = d.wpk + ((long long)i * 9) * cout_pad + og;
        float t[DIRECT_CG];
#pragma unroll
        for (int k = 0; k < DIRECT_CG; k++) t[k] = 0.0f;                                // filter2D delta = 0
#pragma unroll
        for (int tap = 0; tap < 9; tap++)                                               // row-major taps
#pragma unroll
            for (int k = 0; k < DIRECT_CG; k++)
                t[k] = __fadd_rn(t[k], __fmul_rn(wp[tap * cout_pad + k], v[tap]));     // mul, then add
#pragma unroll
        for (int k = 0; k < DIRECT_CG; k++) acc[k] = __fadd_rn(acc[k], t[k]);           // cv::add :144
    }
    float *op = d.out + (long long)y * d.out_rs + (long long)x * d.out_ps;
#pragma unroll
    for (int k = 0; k < DIRECT_CG; k++) {
        if (og + k < d.cout) {
            const float v = __fadd_rn(acc[k], d.bias[og + k]);                           // :147
            const float pos = v > 0.0f ? v : 0.0f, neg = v < 0.0f ? v : 0.0f;            // :150-151
            op[(long long)(og + k) * d.out_cs] = __fadd_rn(__fmul_rn(neg, 0.1f), pos);   // :152
        }
    }
}

// ------------------------------------------------------------------------------------------------
// conv3x3_mfma2: second-generation fp32 MFMA implicit GEMM -- every MFMA operand comes from LDS and
// every byte gets there by LDS-DMA (global_load_lds_dwordx4), so the matrix-core instruction stream
// only ever waits on lgkmcnt; the in-order vmcnt queue holds nothing but bulk transfers issued two
// or more stages ahead and the epilogue stores.
//
//   Persistent workgroup (1 per CU, 4 waves, one per SIMD, up to 512 registers each), tile = 8 rows
//   x 32 pixels x COUT planes; wave (wm, wn) owns MB row-blocks x NB plane-blocks (MB*WM = 8).
//   Stage = (32-channel slice, tap): 4 k-groups of 8 channels = 16*MB*NB MFMAs per wave.
//   LDS:  A[2] x 44 KiB  halo tile (10 x 34 pixels x 32 channels) of the current / next slice,
//                        UNPADDED 128 B per pixel, 16-byte chunk q of pixel p stored at chunk
//                        position q ^ ((p>>1)&7)  (DMA writes are lane-linear, so the swizzle is
//                        applied to the per-lane SOURCE address; ds_read_b128 of 32 consecutive
//                        pixels is then conflict-free in all four 16-lane groups)
//         B[4] x 4*NBT KiB  the weights of one stage in MFMA fragment order (a straight copy of
//                        wpk[tap][4 k-groups][NBT][64 lanes][4]); ring of 4 stages.
//   Schedule at stage t:  issue DMA B(t+3) and up to 2 pieces of A(next slice | next tile);
//   at its end wait (counted vmcnt) for this wave's share of B(t+2) [and A(next) when t = 7],
//   raw s_barrier.  B(t+1) was already complete at the previous barrier, so the first fragments
//   of stage t+1 are read BEFORE the barrier and the MFMA stream runs across it.
// ------------------------------------------------------------------------------------------------

template <int CIN, int COUT, int MB, int NB, int WM, int WN, int EPI = 1>
__global__ void __launch_bounds__(WM *WN * 64, WM *WN / 4) conv3x3_mfma2(W2xcConvDesc d, int tiles_x, int ntiles)
{
    constexpr int NST = MB * NB * 16;                // stores per wave in an interior-tile epilogue
    constexpr int ROWS = 8, HW = 34, HH = ROWS + 2, NPIX = HH * HW;
    constexpr int NSL = CIN / 32, NBT = COUT / 32;
    constexpr int NW = WM * WN;                      // 4 waves (one per SIMD) or 8 (two per SIMD)
    constexpr int APW = (43 + NW) / NW;              // A pieces (1 KiB) per wave per slice: NW*APW >= 42.5
    constexpr unsigned A_BYTES = NW * APW * 1024;    // 45056 (4 waves) / 49152 (8 waves)
    constexpr int BPW = 4 * NBT / NW;                // B pieces per wave per stage (4*NBT in total)
    constexpr unsigned B_BYTES = 4 * NBT * 1024;
    constexpr unsigned B_BASE = 2 * A_BYTES;
    static_assert((NW == 4 || NW == 8) && MB * WM == ROWS && NB * WN == NBT && BPW * NW == 4 * NBT, "tile shape");
    static_assert(CIN % 32 == 0 && COUT % 32 == 0, "planes");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float *)lds;
    const char *ldsb = reinterpret_cast<const char *>(lds);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WN, wn = wave - wm * WN;
    const int nb0 = wn * NB;
    const int li = lane & 31, kk = lane >> 5;

    // persistent schedule: XCD x (= blockIdx % 8) walks its own contiguous chunk of the tile list
    const int xcd = blockIdx.x & 7, per = gridDim.x >> 3;
    const int cq = ntiles >> 3, cr = ntiles & 7;
    const int chunk_begin = xcd < cr ? xcd * (cq + 1) : cr * (cq + 1) + (xcd - cr) * cq;
    const int chunk_end = chunk_begin + cq + (xcd < cr ? 1 : 0);
    int tile = chunk_begin + (blockIdx.x >> 3);
    if (tile >= chunk_end) return;

    float bv[NB];
#pragma unroll
    for (int nb = 0; nb < NB; nb++) bv[nb] = d.bias[(nb0 + nb) * 32 + li];

    // ---- per-lane DMA source offsets of the A halo tile (16-byte units), piece jj of this wave ----
    const f32x4 *in4 = reinterpret_cast<const f32x4 *>(d.in);
    // goff[jj] = lofs[jj] + (tile origin) for tiles whose halo needs no clamping (all but the border tiles):
    // lofs is tile-independent, so the per-tile bookkeeping is APW adds instead of ~20 VALU per piece.
    unsigned goff[APW], lofs[APW];
#pragma unroll
    for (int jj = 0; jj < APW; jj++) {
        const int s = (jj * NW + wave) * 64 + lane;
        int p = s >> 3;
        p = p < NPIX ? p : NPIX - 1;
        const int py = p / HW, px = p - py * HW;
        lofs[jj] = (unsigned)(((long long)py * d.in_rs + (long long)px * CIN) >> 2) + ((s & 7) ^ ((p >> 1) & 7));
    }
    auto tile_offsets = [&](int t) {
        const int ty_ = t / tiles_x, tx_ = t - ty_ * tiles_x;
        const int y0 = ty_ * ROWS + d.off_y, x0 = tx_ * 32 + d.off_x;
        if (y0 >= 0 && y0 + HH <= d.in_h && x0 >= 0 && x0 + HW <= d.in_w) {   // wave-uniform
            const unsigned base = (unsigned)(((long long)y0 * d.in_rs + (long long)x0 * CIN) >> 2);
#pragma unroll
            for (int jj = 0; jj < APW; jj++) goff[jj] = lofs[jj] + base;
            return;
        }
#pragma unroll
        for (int jj = 0; jj < APW; jj++) {
            const int s = (jj * NW + wave) * 64 + lane;           // 16-byte slot in the A buffer
            int p = s >> 3;
            p = p < NPIX ? p : NPIX - 1;                           // slots past the tile re-read its last pixel
            const int q = (s & 7) ^ ((p >> 1) & 7);                // chunk stored at this position
            const int py = p / HW, px = p - py * HW;
            const int gy = clampi(y0 + py, 0, d.in_h - 1);
            const int gx = clampi(x0 + px, 0, d.in_w - 1);
            goff[jj] = (unsigned)(((long long)gy * d.in_rs + (long long)gx * CIN) >> 2) + q;
        }
    };
    const unsigned b_voff = (unsigned)((wave * BPW) * 64 + lane) * 16u;                      // this wave's B pieces
    auto dma_b = [&](int sl_, int tap_, unsigned buf, int jb) {   // piece jb of stage (sl_, tap_) -> ring slot buf
        const char *sbase = reinterpret_cast<const char *>(d.wpk) + (size_t)(tap_ * (CIN / 8) + sl_ * 4) * NBT * 1024;
        const unsigned dst = lds0 + B_BASE + buf * B_BYTES + (unsigned)(wave * BPW) * 1024u;
        switch (jb) {
        case 0: lds_dma16_s<0>(sbase, b_voff, dst); break;
        // the instruction's immediate offset is applied to BOTH the global and the LDS address
        case 1: lds_dma16_s<1024>(sbase, b_voff, dst); break;
        case 2: lds_dma16_s<2048>(sbase, b_voff, dst); break;
        default: lds_dma16_s<3072>(sbase, b_voff, dst); break;
        }
    };
    auto dma_a = [&](unsigned add, unsigned abuf, int jj) {
        lds_dma16(in4 + goff[jj] + add, lds0 + abuf * A_BYTES + (unsigned)(jj * NW + wave) * 1024u);
    };

    // ---- fragment addressing ----
    // A: lane (li, kk) reads chunk q = 2*c8 + kk of pixel p = (wm*MB + row)*34 + li + tx, row = mb + ty:
    //    byte p*128 + ((q ^ ((p>>1)&7)) << 4) = a0[row][tx] ^ (c8 << 5)  with a0 the c8 = 0 address
    //    (bits 0..6 of p*128 are zero and 2*c8 only touches chunk bits 1..2).  a0 is tile-independent.
    unsigned a0[MB + 2][3];
#pragma unroll
    for (int row = 0; row < MB + 2; row++)
#pragma unroll
        for (int tx = 0; tx < 3; tx++) {
            const int p = (wm * MB + row) * HW + li + tx;
            a0[row][tx] = (unsigned)(p * 128 + ((((p >> 1) & 7) ^ kk) << 4));
        }
    auto a_addr = [&](unsigned abuf, int mb, int tap, int c8) -> const f32x4 * {
        return reinterpret_cast<const f32x4 *>(ldsb + ((a0[mb + tap / 3][tap % 3] ^ (unsigned)(c8 << 5)) + abuf * A_BYTES));
    };
    auto b_addr = [&](unsigned buf, int c8, int nb) -> const f32x4 * {
        return reinterpret_cast<const f32x4 *>(ldsb + B_BASE + buf * B_BYTES + ((c8 * NBT + nb0 + nb) * 64 + lane) * 16);
    };

    f32x16 acc[MB][NB];
#pragma unroll
    for (int mb = 0; mb < MB; mb++)
#pragma unroll
        for (int nb = 0; nb < NB; nb++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[mb][nb][r] = 0.0f;

    // ---- prologue: A(slice 0) and B stages 0..2 of the first tile ----
    tile_offsets(tile);
#pragma unroll
    for (int jj = 0; jj < APW; jj++) dma_a(0, 0, jj);
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
        for (int jb = 0; jb < BPW; jb++) dma_b((t / 9) % NSL, t % 9, t & 3, jb);
    W2XC_WAIT_VMCNT(0);
    __builtin_amdgcn_s_barrier();

    unsigned gs = 0;      // global stage counter (only gs & 3 matters): ring slot of the current stage
    unsigned abuf = 0;    // A buffer of the current slice
    int sl = 0;
    bool epi_stores = false;   // an interior-tile epilogue (NST stores) directly precedes the current stage
    f32x4 a_cur[MB], b_cur[NB];
#pragma unroll
    for (int mb = 0; mb < MB; mb++) a_cur[mb] = *a_addr(0, mb, 0, 0);
#pragma unroll
    for (int nb = 0; nb < NB; nb++) b_cur[nb] = *b_addr(0, 0, nb);

    for (;;) {
        // what the A pieces issued during this slice fetch: the next slice, or the next tile's first
        const bool last_slice = (sl == NSL - 1);
        unsigned a_add = (unsigned)(sl + 1) * 8;
        if (last_slice) {
            tile_offsets(tile + per < chunk_end ? tile + per : tile);
            a_add = 0;
        }
        const int sl_next = last_slice ? 0 : sl + 1;

#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            // stage (sl, tap) in ring slot gs&3; DMA targets: B of stage +3, A pieces 2 per stage on taps 0..5
            const int tap3 = (tap + 3) % 9;
            const int sl3 = (tap + 3 < 9) ? sl : sl_next;
            const unsigned buf = gs & 3u, buf3 = (gs + 3u) & 3u, buf1 = (gs + 1u) & 3u;
            // A pieces of the next slice are issued on taps 0..5: KA[t] = ceil-spread of APW over 6 stages
            constexpr int KA[9] = {(APW + 5) / 6, (APW + 4) / 6, (APW + 3) / 6, (APW + 2) / 6, (APW + 1) / 6, APW / 6, 0, 0, 0};
            int ja0 = 0;               // first A piece of this stage
#pragma unroll
            for (int t = 0; t < 9; t++) ja0 += t < tap ? KA[t] : 0;
#pragma unroll
            for (int c8 = 0; c8 < 4; c8++) {
                // One step = M MFMAs.  Every other instruction is pinned into an MFMA shadow:
                //   the MB + NB fragment reads of the NEXT step (the last step of a stage reads the next
                //   stage's first fragments, which the previous barrier already guaranteed), spaced evenly;
                //   the DMAs: step 0: [A piece, A piece,] B piece 0; steps 1..3: B piece c8.
                constexpr int M = 4 * MB * NB, R = MB + NB;
                const bool wrap = (c8 == 3);
                const int tap_n = wrap ? (tap + 1) % 9 : tap, c8_n = wrap ? 0 : c8 + 1;
                const unsigned abuf_n = (wrap && tap == 8) ? (abuf ^ 1u) : abuf;
                const unsigned bbuf_n = wrap ? buf1 : buf;
                f32x4 a_nxt[MB], b_nxt[NB];
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int mb = 0; mb < MB; mb++)
#pragma unroll
                        for (int nb = 0; nb < NB; nb++) {
                            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[mb][j], b_cur[nb][j], acc[mb][nb], 0, 0, 0);
                            const int m = (j * MB + mb) * NB + nb;        // MFMA index in the step
                            if (c8 == 0 && (m == 1 || m == 3) && (m >> 1) < KA[tap]) {
                                __builtin_amdgcn_sched_barrier(0);
                                dma_a(a_add, abuf ^ 1u, ja0 + (m >> 1));
                                __builtin_amdgcn_sched_barrier(0);
                            }
                            if (m == (c8 == 0 ? 5 : 1) && c8 < BPW) {
                                __builtin_amdgcn_sched_barrier(0);
                                dma_b(sl3, tap3, buf3, c8);
                                __builtin_amdgcn_sched_barrier(0);
                            }
#pragma unroll
                            for (int r = 0; r < R; r++) {
                                if (m == 1 + (r * (M - 5)) / R) {         // reads spread over MFMAs 1 .. M-5: >= 4 MFMAs cover the LDS latency
                                    __builtin_amdgcn_sched_barrier(0);
                                    if (r < MB) a_nxt[r] = *a_addr(abuf_n, r, tap_n, c8_n);
                                    else b_nxt[r - MB] = *b_addr(bbuf_n, c8_n, r - MB);
                                    __builtin_amdgcn_sched_barrier(0);
                                }
                            }
                        }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mb = 0; mb < MB; mb++) a_cur[mb] = a_nxt[mb];
#pragma unroll
                for (int nb = 0; nb < NB; nb++) b_cur[nb] = b_nxt[nb];
            }
            // stage boundary.  The youngest transfer needed next is this wave's last piece of B(t+2),
            // issued in stage t-1 after that stage's A pieces; the only younger transfers are the
            // KA[t] + BPW issued in stage t (vmcnt retires in order; the epilogue stores of the
            // previous tile, if any, are older than stage t's transfers and are retired too).
            {
                // After an interior-tile epilogue exactly NST stores sit in the queue between B(t+2) and
                // stage t's transfers: counting them in lets the stores drain under the next two stages
                // instead of stalling the first one (n >= 63 = queue depth: nothing to wait for).
                const int n_dma = KA[tap] + BPW;
                if (EPI && tap == 0 && epi_stores) wait_vmcnt_n(n_dma + NST);
                else wait_vmcnt_n(n_dma);
                if (tap == 0) epi_stores = false;
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
            gs++;
        }
        abuf ^= 1u;

        if (last_slice) {
            // ---- epilogue: bias + LeakyReLU, NHWC stores (C/D: column = lane&31, row = (r&3)+8*(r>>2)+4*(lane>>5)).
            //      leaky(v) = max(v, 0.1f*v).  Interior tiles (all but the last row / column of tiles)
            //      take the unpredicated path. ----
            const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
            const int oy0 = tile_y * ROWS, ox0 = tile_x * 32;
            const bool interior = (oy0 + ROWS <= d.out_h) && (ox0 + 32 <= d.out_w);
            float *obase = d.out + (long long)(oy0 + wm * MB) * d.out_rs + (long long)(ox0 + 4 * kk) * COUT + nb0 * 32 + li;
            if (interior) {
#pragma unroll
                for (int mb = 0; mb < MB; mb++)
#pragma unroll
                    for (int nb = 0; nb < NB; nb++)
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const float v = acc[mb][nb][r] + bv[nb];
                            obase[(long long)mb * d.out_rs + ((r & 3) + 8 * (r >> 2)) * COUT + nb * 32] = __builtin_amdgcn_fmed3f(v, 0.1f * v, 3.402823466e+38f);
                            acc[mb][nb][r] = 0.0f;
                        }
                epi_stores = true;
            } else {
#pragma unroll
                for (int mb = 0; mb < MB; mb++) {
                    const int y = oy0 + wm * MB + mb;
#pragma unroll
                    for (int nb = 0; nb < NB; nb++)
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const int x = ox0 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                            const float v = acc[mb][nb][r] + bv[nb];
                            if (y < d.out_h && x < d.out_w)
                                obase[(long long)mb * d.out_rs + ((r & 3) + 8 * (r >> 2)) * COUT + nb * 32] = __builtin_amdgcn_fmed3f(v, 0.1f * v, 3.402823466e+38f);
                            acc[mb][nb][r] = 0.0f;
                        }
                }
            }
            tile += per;
            if (tile >= chunk_end) break;
            sl = 0;
        } else {
            sl++;
        }
    }
    W2XC_WAIT_VMCNT(0);   // drain the speculative DMAs before the LDS is released
}

// ------------------------------------------------------------------------------------------------
// conv3x3_first: cin <= 3, planar input, cout = 32*NBT planes, NHWC output.
//   K = 9*CIN (k = c*9 + tap), padded to 2*S; lane (i, kk) feeds k = 2*s + kk of MFMA step s.
//   Packed weights: wpk[nb][s][lane] = W[32*nb + (lane&31)][c][tap] for k = 2*s + (lane>>5) < K, else 0.
//   Workgroup = 4 waves, tile = 8 rows x 32 pixels; wave w owns rows 2w, 2w+1.
// ------------------------------------------------------------------------------------------------
#ifndef FIRST_TPW
#define FIRST_TPW 4
#endif
// U8 (W2XC_K_FIRST_U8): the source is an interleaved uint8 image -- d.in points at BYTES, in_rs / in_ps / in_cs are byte strides (row stride, 3, 1; or
// row stride, 4, 0 with d.in at an RGBA image's alpha byte: the three planes are then that byte, the grey image (A, A, A) without its copy) -- and the
// patch load converts, (float)byte * (float)(1.0 / 255.0): the expression of the colour kernels (w2xc_color.hip), so the float planes they would write for
// this layer to read never exist.  Everything behind the patch load is the float form's.
template <int CIN, int NBT, bool PLANAR = false, bool U8 = false>
__global__ void __launch_bounds__(256) conv3x3_first(W2xcConvDesc d, int tiles_x, int ntiles)
{
#define FLB_ONLY(...)
#define FLB_SEL(b_, s_) s_
#define FLB_IN d.in
#define FLB_OUT d.out
#include "w2xc_first_body.inc"
#undef FLB_OUT
#undef FLB_IN
#undef FLB_SEL
#undef FLB_ONLY
}

// ------------------------------------------------------------------------------------------------
// conv3x3_last: cout <= 3, NHWC input, planar output.  "Taps as N".
//   For each haloed pixel q of the tile: G[q][n] = sum_c in[q][c] * W[o][c][tap], n = tap*COUT + o,
//   N = 9*COUT padded to 16*NB16, on v_mfma_f32_16x16x4_f32 (M = 16 pixels, K = 4).  A comes
//   straight from global memory: lane (i = lane&15, kk = lane>>4) loads channels
//   16*s4 + 4*kk .. +3 of pixel i as one dwordx4; MFMA j of group s4 contracts channels
//   {16*s4 + 4*kk + j}.  Packed weights: wpk[s4][j][nb][lane] = W[o][16*s4 + 4*(lane>>4) + j][tap]
//   for n = 16*nb + (lane&15) = tap*COUT + o < 9*COUT, else 0.
//   Then out[p][o] = leaky(bias[o] + sum_tap G[p + tap][tap*COUT + o]) via LDS.
//   Workgroup = 4 waves, tile = ROWS x 32 output pixels.
// ------------------------------------------------------------------------------------------------
#ifndef LAST_TPW
#define LAST_TPW 4
#endif
// U8 (W2XC_K_LAST_U8): the sink is an interleaved uint8 image -- d.out points at BYTES, out_rs / out_ps / out_cs are byte strides (row stride, COUT, 1) -- and
// the epilogue stores saturate(rint(255 v)) with the rounding of the colour kernels (w2xc_color.hip): one byte store per value, so a thread writes its own
// bytes only (the neighbours are other threads' or, with an ROI as output, the caller's).
template <int CIN, int COUT, bool U8 = false>
__global__ void __launch_bounds__(256) conv3x3_last(W2xcConvDesc d, int tiles_x, int ntiles)
{
#define FLB_ONLY(...)
#define FLB_SEL(b_, s_) s_
#define FLB_IN d.in
#define FLB_OUT d.out
#include "w2xc_last_body.inc"
#undef FLB_OUT
#undef FLB_IN
#undef FLB_SEL
#undef FLB_ONLY
}

// replicate-padded planar copy: dst plane c (ph x pw pixels, row stride d_rs, plane stride d_cs) = src(clamp(y - pad), clamp(x - pad)) -- the
// BORDER_REPLICATE of Model::filter (modelHandler.cpp:141-142) made explicit for the kernels that run a valid conv on aligned planar tiles
__global__ void __launch_bounds__(256) pad_planar_kernel(const float *src, long long s_rs, long long s_ps, long long s_cs, float *dst, long long d_rs,
                                                         long long d_cs, int h, int w, int c, int pad)
{
    const int pw = w + 2 * pad, ph = h + 2 * pad;
    const long long total = (long long)c * ph * pw;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int x = (int)(idx % pw);
        const long long r = idx / pw;
        const int y = (int)(r % ph), ch = (int)(r / ph);
        const int sy = clampi(y - pad, 0, h - 1), sx = clampi(x - pad, 0, w - 1);
        dst[(long long)ch * d_cs + (long long)y * d_rs + x] = src[(long long)ch * s_cs + (long long)sy * s_rs + (long long)sx * s_ps];
    }
}

// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) repack_kernel(const float *src, long long s_rs, long long s_ps, long long s_cs,
                                                     float *dst, long long d_rs, long long d_ps, long long d_cs,
                                                     int h, int w, int c)
{
    const long long total = (long long)h * w * c;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int ch = (int)(idx % c);
        const long long p = idx / c;
        const int x = (int)(p % w), y = (int)(p / w);
        dst[y * d_rs + x * d_ps + ch * d_cs] = src[y * s_rs + x * s_ps + ch * s_cs];
    }
}

// ================================================================================================
// host side: launch (kernel selection and the weight packers: w2xc_pack.cpp)
// ================================================================================================
template <int CIN, int COUT, int MB, int NB, int WM, int WN>
static hipError_t launch_mfma2(const W2xcConvDesc &d, hipStream_t stream)
{
    const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + 7) / 8;
    const int ntiles = tiles_x * tiles_y;
    constexpr int NW = WM * WN;
    const size_t lds_bytes = 2 * (size_t)(NW * ((43 + NW) / NW) * 1024) + 4 * (size_t)(4 * (COUT / 32) * 1024);
    auto kern = conv3x3_mfma2<CIN, COUT, MB, NB, WM, WN>;
    static W2xcLdsOptIn opt_in;   // per (kernel, device)
    const hipError_t e = opt_in(kern, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(w2xc_persistent_grid(ntiles)), dim3(NW * 64), lds_bytes, stream, d, tiles_x, ntiles);
    return hipGetLastError();
}

template <typename KernelT>
static hipError_t launch_tiled8(KernelT kernel, const W2xcConvDesc &d, hipStream_t stream)
{
    const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + 7) / 8;
    const int ntiles = tiles_x * tiles_y;
    hipLaunchKernelGGL(kernel, dim3(ntiles), dim3(256), 0, stream, d, tiles_x, ntiles);
    return hipGetLastError();
}

template <typename KernelT>
static hipError_t launch_last(KernelT kernel, const W2xcConvDesc &d, hipStream_t stream)
{
    const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + 7) / 8;
    const int ntiles = tiles_x * tiles_y;
    hipLaunchKernelGGL(kernel, dim3((ntiles + LAST_TPW - 1) / LAST_TPW), dim3(256), 0, stream, d, tiles_x, ntiles);
    return hipGetLastError();
}

template <typename KernelT>
static hipError_t launch_first(KernelT kernel, const W2xcConvDesc &d, hipStream_t stream)
{
    const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + 7) / 8;
    const int ntiles = tiles_x * tiles_y;
    hipLaunchKernelGGL(kernel, dim3((ntiles + FIRST_TPW - 1) / FIRST_TPW), dim3(256), 0, stream, d, tiles_x, ntiles);
    return hipGetLastError();
}

hipError_t w2xc_launch_conv(W2xcKernelKind kind, const W2xcConvDesc &d, hipStream_t stream)
{
    if (d.out_w <= 0 || d.out_h <= 0) return hipSuccess;
    if (d.in_shift != 0 && kind != W2XC_K_FIRST && kind != W2XC_K_FIRST_U8 && kind != W2XC_K_DIRECT) return hipErrorInvalidValue;
    if (kind == W2XC_K_MFMA) {
        if (d.in_ps != d.cin || d.in_cs != 1 || d.out_ps != d.cout || d.out_cs != 1) return hipErrorInvalidValue;
        const int key = d.cin * 1000 + d.cout;
        // Measured inside the 7-layer model (round 2, same box, same run): 8 waves (two per SIMD: the partner's MFMAs cover
        // this wave's non-MFMA issue slots) win wherever the output has >= 64 planes (32->64 -1.8 %, 64->64 -2.5 %,
        // 64->128 -2.9 %, 128->128 -2.9 %); 32->32 has one plane block, so its 8 waves would split rows only.
        const bool w8 = d.cout >= 64;
        switch (key) {
        //                                  CIN  COUT  MB NB WM WN
        case 32032:  return launch_mfma2<32, 32, 2, 1, 4, 1>(d, stream);
        case 32064:  return w8 ? launch_mfma2<32, 64, 2, 1, 4, 2>(d, stream) : launch_mfma2<32, 64, 2, 2, 4, 1>(d, stream);
        case 32128:  return w8 ? launch_mfma2<32, 128, 2, 2, 4, 2>(d, stream) : launch_mfma2<32, 128, 4, 2, 2, 2>(d, stream);
        case 64032:  return launch_mfma2<64, 32, 2, 1, 4, 1>(d, stream);
        case 64064:  return w8 ? launch_mfma2<64, 64, 2, 1, 4, 2>(d, stream) : launch_mfma2<64, 64, 2, 2, 4, 1>(d, stream);
        case 64128:  return w8 ? launch_mfma2<64, 128, 2, 2, 4, 2>(d, stream) : launch_mfma2<64, 128, 4, 2, 2, 2>(d, stream);
        case 128032: return launch_mfma2<128, 32, 2, 1, 4, 1>(d, stream);
        case 128064: return w8 ? launch_mfma2<128, 64, 2, 1, 4, 2>(d, stream) : launch_mfma2<128, 64, 2, 2, 4, 1>(d, stream);
        case 128128: return w8 ? launch_mfma2<128, 128, 2, 2, 4, 2>(d, stream) : launch_mfma2<128, 128, 4, 2, 2, 2>(d, stream);
        default: return hipErrorInvalidValue;
        }
    }
    if (kind == W2XC_K_FIRST_U8) {   // three interleaved uint8 channels in; either output layout, with the float form's conditions
        if (d.cin != 3 || !((d.in_ps == 3 && d.in_cs == 1) || (d.in_ps == 4 && d.in_cs == 0))) return hipErrorInvalidValue;   // (4, 0: the alpha byte of RGBA pixels as all three planes)
        if (d.out_ps == 1) {
            if (((d.out_rs | d.out_cs) & 3) != 0 || d.out_rs < ((d.out_w + 3) & ~3) || (((size_t)d.out) & 15) != 0) return hipErrorInvalidValue;
            switch (d.cout) {
            case 32: return launch_first(conv3x3_first<3, 1, true, true>, d, stream);
            case 64: return launch_first(conv3x3_first<3, 2, true, true>, d, stream);
            case 128: return launch_first(conv3x3_first<3, 4, true, true>, d, stream);
            default: return hipErrorInvalidValue;
            }
        }
        if (d.out_ps != d.cout || d.out_cs != 1) return hipErrorInvalidValue;
        switch (d.cout) {
        case 32: return launch_first(conv3x3_first<3, 1, false, true>, d, stream);
        case 64: return launch_first(conv3x3_first<3, 2, false, true>, d, stream);
        case 128: return launch_first(conv3x3_first<3, 4, false, true>, d, stream);
        default: return hipErrorInvalidValue;
        }
    }
    if (kind == W2XC_K_LAST_U8) {   // three interleaved uint8 channels out
        if (d.in_ps != d.cin || d.in_cs != 1 || d.cout != 3 || d.out_ps != 3 || d.out_cs != 1) return hipErrorInvalidValue;
        switch (d.cin) {
        case 32: return launch_last(conv3x3_last<32, 3, true>, d, stream);
        case 64: return launch_last(conv3x3_last<64, 3, true>, d, stream);
        case 128: return launch_last(conv3x3_last<128, 3, true>, d, stream);
        default: return hipErrorInvalidValue;
        }
    }
    if (kind == W2XC_K_FIRST && d.out_ps == 1 && d.cout > 1) {   // planar out: whole pixel quads (the engine's planar workspaces; Model::filter goes through NHWC)
        if (((d.out_rs | d.out_cs) & 3) != 0 || d.out_rs < ((d.out_w + 3) & ~3) || (((size_t)d.out) & 15) != 0) return hipErrorInvalidValue;
        switch (d.cin * 1000 + d.cout) {
        case 1032: return launch_first(conv3x3_first<1, 1, true>, d, stream);
        case 1064: return launch_first(conv3x3_first<1, 2, true>, d, stream);
        case 1128: return launch_first(conv3x3_first<1, 4, true>, d, stream);
        case 3032: return launch_first(conv3x3_first<3, 1, true>, d, stream);
        case 3064: return launch_first(conv3x3_first<3, 2, true>, d, stream);
        case 3128: return launch_first(conv3x3_first<3, 4, true>, d, stream);
        default: return hipErrorInvalidValue;
        }
    }
    if (kind == W2XC_K_FIRST) {
        if (d.out_ps != d.cout || d.out_cs != 1) return hipErrorInvalidValue;
        const int key = d.cin * 1000 + d.cout;
        switch (key) {
        case 1032: return launch_first(conv3x3_first<1, 1>, d, stream);
        case 1064: return launch_first(conv3x3_first<1, 2>, d, stream);
        case 1128: return launch_first(conv3x3_first<1, 4>, d, stream);
        case 3032: return launch_first(conv3x3_first<3, 1>, d, stream);
        case 3064: return launch_first(conv3x3_first<3, 2>, d, stream);
        case 3128: return launch_first(conv3x3_first<3, 4>, d, stream);
        default: return hipErrorInvalidValue;
        }
    }
    if (kind == W2XC_K_LAST) {
        if (d.in_ps != d.cin || d.in_cs != 1) return hipErrorInvalidValue;
        const int key = d.cin * 1000 + d.cout;
        switch (key) {
        case 32001:  return launch_last(conv3x3_last<32, 1>, d, stream);
        case 64001:  return launch_last(conv3x3_last<64, 1>, d, stream);
        case 128001: return launch_last(conv3x3_last<128, 1>, d, stream);
        case 32003:  return launch_last(conv3x3_last<32, 3>, d, stream);
        case 64003:  return launch_last(conv3x3_last<64, 3>, d, stream);
        case 128003: return launch_last(conv3x3_last<128, 3>, d, stream);
        default: return hipErrorInvalidValue;
        }
    }
    const int cp = direct_cout_pad(d.cout);
    dim3 grid((d.out_w + 63) / 64, (d.out_h + 3) / 4, cp / DIRECT_CG);
    hipLaunchKernelGGL(conv3x3_direct, grid, dim3(64, 4), 0, stream, d, cp);
    return hipGetLastError();
}

hipError_t w2xc_launch_pad_planar(const float *src, long long s_rs, long long s_ps, long long s_cs, float *dst, long long d_rs, long long d_cs,
                                  int h, int w, int c, int pad, hipStream_t stream)
{
    const long long total = (long long)c * (h + 2 * pad) * (w + 2 * pad);
    if (total <= 0) return hipSuccess;
    long long blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(pad_planar_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, s_rs, s_ps, s_cs, dst, d_rs, d_cs, h, w, c, pad);
    return hipGetLastError();
}

hipError_t w2xc_launch_repack(const float *src, long long s_rs, long long s_ps, long long s_cs, float *dst,
                              long long d_rs, long long d_ps, long long d_cs, int h, int w, int c, hipStream_t stream)
{
    const long long total = (long long)h * w * c;
    if (total <= 0) return hipSuccess;
    long long blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(repack_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, s_rs, s_ps, s_cs, dst, d_rs,
                       d_ps, d_cs, h, w, c);
    return hipGetLastError();
}
