// w2xc_wino4.hip -- conv3x3_wino4: the 3x3 x Cin x Cout contraction of Model::filterWorker
// (/root/reference/src/modelHandler.cpp:117-159) as Winograd F(4x4, 3x3) on v_mfma_f32_16x16x4_f32, two waves per SIMD,
// on PLANAR activations (one H x W fp32 plane per channel -- the reference's own std::vector<cv::Mat> layout).
//
//   Y = A^T [ (G g G^T) (.) (B^T d B) ] A   per 4x4 output block and 6x6 input patch: 36 positions xi of the transformed domain =
//   36 independent GEMMs  M_xi[o][t] = sum_c U_xi[o][c] V_xi[c][t]  (o = output plane, t = block, c = input plane): 2.25 multiplies
//   per output.  fp32 throughout; Cook-Toom on the points 0, +-3/4, +-3/2, inf (tools/winograd_points.py: every entry a dyadic rational):
//     B^T = [81/64 0 -45/16 0 1 0; 0 -27/16 -9/4 3/4 1 0; 0 27/16 -9/4 -3/4 1 0; 0 -27/32 -9/16 3/2 1 0; 0 27/32 -9/16 -3/2 1 0; 0 81/64 0 -45/16 0 1]
//     G   = [64/81 0 0; -128/243 -32/81 -8/27; -128/243 32/81 -8/27; 32/243 16/81 8/27; 32/243 -16/81 8/27; 0 0 1]
//     A^T = [1 1 1 1 1 0; 0 3/4 -3/4 3/2 -3/2 0; 0 9/16 9/16 9/4 9/4 0; 0 27/64 -27/64 27/8 -27/8 1]
//
//   Work item  16 rows x 32 pixels of output (4 x 8 blocks of 4x4) x 64 output planes.  8 waves: wave (bt, pt) owns block tile bt
//              (block rows 2 bt, 2 bt + 1) x plane tile pt (16 planes) x all 36 xi = 144 accumulators.
//   Stage      one 4-CHANNEL slice = the K of one MFMA: 36 MFMAs per wave, both operands from LDS in fragment order
//              [xi / 4][tile][lane][xi % 4] (one ds_read_b128 per four xi and operand, read two groups of four MFMAs ahead; A = U, lane = 16 k + o;
//              B = V, lane = 16 k + t).  The stage's closing wait + barrier sit in FRONT of its last four MFMAs: behind the barrier a wave reads the
//              first operands of the next stage and still has four MFMAs to issue while they arrive.  An item's first stage is its own copy of the
//              stage body: its MFMAs take 0 as accumulator input (no zeroing of 144 registers per wave and item).
//   V          is computed once per (block, channel) and shared by the four plane-tile waves through LDS.  ONE wave transforms a 4-channel slice of
//              its block tile in FOUR QUARTERS over four consecutive stages, the 36 values in REGISTERS in between (Q0 raw patch + row pass of rows
//              0..2 | Q1 rows 3..5 | Q2 column pass of columns 0..2 | Q3 columns 3..5 + nine ds_write_b128 of V): every wave carries the same 42 VALU
//              instructions in every stage, the four waves of a block tile are one quarter apart, the two waves of a SIMD two.  The pipeline runs
//              across items; the waves in mid-transform at an item's end keep their 36 values in registers across the epilogue (the PROG forms, whose
//              epilogue calls a function, park them in LDS).  V is two slots.
//              The MFMAs are asm with the accumulator TIED: as builtins the allocator gave three of four a destination other than their
//              accumulator input, the accumulators migrated through the file and some were spilled inside the stages.
//   LDS        raw[3] x 11 KiB: the 18 x 36 pixel halo tile of a 4-channel slice as 16-byte chunks (channel kk, row R, pixel quad q) at
//              chunk index kk * 168 + R * 9 + q (the stride 168 = 8 mod 16 makes the b128 patch reads conflict-free);
//              U[2] x 36 KiB + V[2] x 18 KiB + 18 KiB + bias = 159.5 KiB.  U slot 1, V slot 1 and the last 18 KiB are idle across an epilogue: 72 KiB =
//              the fused last layer's tap exchange of a whole item (PROG: U slot 1 + the 18 KiB park the transforms, V slot 1 is the exchange of one row step).
//   Transfers  LDS-DMA (global_load_lds_dwordx4), SGPR base + 32-bit lane offset: per stage 36 U pieces (one stage ahead) and 11 raw
//              pieces (the slice Q0 reads two stages later; the closing wait of a stage leaves its own raw pieces in flight), all issued by the
//              four OLDER waves: they win the matrix pipe's arbitration and have the time (W4_DMA4).  A lane's 16 bytes are four
//              consecutive pixels of one plane row: whole 128-byte lines (the engine gives planar rows a stride of roundup32(w) floats).
//   32 planes in  (IN_NHWC) the producers conv3x3_first / conv3x3_wino write NHWC pixels of one 128-byte line: a raw chunk is then the four
//              channels of ONE pixel, the pixels of a row grouped by column mod 4 (conflict-free ds_read_b32 of a lane's channel).
//   Epilogue   Y = A^T M A per output-row pair, bias, LeakyReLU; planar out: one 16-byte store = four pixels of a plane row, 8 lanes = one
//              128-byte line (NHWC out for a consumer that wants it).  FUSE7: the model's one-plane LAST layer on the activations just
//              computed ("taps as rows" on the MFMA), the four plane tiles of a block summed through idle LDS, the item in one piece: 9 partial tap planes
//              per 64-plane block leave the chip (72 B per pixel instead of 512), conv3x3_last_gather finishes.
//   Edges      rows are clamped (replicate) in the transfer addresses; patch columns >= in_w are ZEROED in the row pass (they only reach
//              outputs >= out_w, and what is in memory there is not defined): results do not depend on memory contents outside the plane.
//   Banding    blocks sit on rows = 0 mod 4 of the layer's whole output (W2xcConvDesc::wino_py = first row mod 4); run_rows' four-rows-per-layer
//              band geometry makes every region edge that is not a plane edge a block edge: bit-identical results across bandings.
// Measured (round 4, 2160x3840, one MI355X): 128 -> 128 6.4-6.8 ms (round 3's NHWC kernel: 7.5 on the same box), frame 14.4-14.9 ms (16.4).  s_memtime: a
// stage takes ~3350 cycles (2304 = the matrix pipe's time for the 72 MFMAs of a SIMD; a synthetic loop of the same shape without transfers: 2670), an
// item's boundary another ~8k of its 116k (profiles/r4_sweeps.log).
// Kernels and launchers only: the shape predicates, PROG's job arithmetic and the weight images (w2xc_wino4_pack, w2xc_wino4_pack_last) are in w2xc_pack.cpp,
// xi_of in w2xc_layout.h, bt6 / at6 in w2xc_wino4_math.h.
#include "w2xc_kernels.h"
#include "w2xc_device.h"
#include "w2xc_launch.hpp"
#include "w2xc_layout.h"
#include "w2xc_wino4_math.h"

#include <type_traits>

#ifdef W4_TIMING
// tools/ubench/wino4_timing.hip: s_memtime stamps of waves 0 and 4 of workgroup 0 -- per stage (before the closing wait, after it, after the
// barrier) and after every epilogue -- [wave >> 2][index]
__device__ unsigned long long w4_stamps[2][8192];
#define W4_STAMP(idx) do { const int i_ = (idx); if (blockIdx.x == 0 && pt == 0 && lane == 0 && i_ < 8192) w4_stamps[bt][i_] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define W4_STAMP(idx) do { } while (0)
#endif
#ifndef W4P_T0
#define W4P_T0 3     // MFMA slot of a stage behind which a wave's transform arithmetic starts (its LDS reads sit behind slot 0)
#endif
#ifndef W4_PF
#define W4_PF 2      // operand look-ahead in groups of four MFMAs (1: two register buffers, 2: three)
#endif
#ifndef W4_DMA4
#define W4_DMA4 1    // 1: the four OLDER waves (block tile 0) issue every transfer (nine U pieces + two / three raw pieces each per stage), the younger four none
#endif
#ifndef W4_ABL
#define W4_ABL 0   // timing-only ablations (wrong results): 1 no transform arithmetic | 2 no transform at all | 16 no U transfers | 32 no raw transfers | 64 no epilogue stores | 128 no operand reads inside the stages
#endif

namespace {

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte global access on a dword-aligned address

// register (dd[6 i + j]) of the value at position xi of the fragment order (xi_of(i, j): w2xc_layout.h)
static constexpr __host__ __device__ int w4p_dd_of(int xi) { return 6 * ((xi % 18) / 3) + 3 * (xi / 18) + (xi % 18) % 3; }

}   // namespace

// 16-byte / 4-byte global stores written THROUGH to memory at device scope (sc1): what another workgroup of this launch, on any XCD, reads after
// the writer has drained them (s_waitcnt vmcnt(0)) and counted its arrival -- no release fence, the XCD's L2 keeps no dirty line (PROG below)
static __device__ __forceinline__ void store16_sc1(float *p, f32x4 v) { asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory"); }
static __device__ __forceinline__ void store4_sc1(float *p, float v) { asm volatile("global_store_dword %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory"); }
// ... and at SYSTEM scope (sc0 sc1): the gather jobs' output rows, which the host pipeline's drainer reads from page-locked host memory as soon as the job's flag
// says so.  Plain stores stayed in the XCD's L2 until the launch ended -- fine-grained host memory is only promised at system-scope synchronisation -- and the
// flag (a system-scope store) arrived long before the rows it announced (measured: stale rows in a third of the frame).
static __device__ __forceinline__ void store16_sys(float *p, f32x4 v) { asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory"); }
static __device__ __forceinline__ void store4_sys(float *p, float v) { asm volatile("global_store_dword %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory"); }

// a batch of N 16-byte sc1 loads (scalar base b[k] + one 32-bit lane offset) issued back to back, and the "+v" pins that keep every destination
// behind the batch's wait (an asm load's destination counts as written at the end of its statement: nothing may read or move it before the wait)
template <int K, int N>
static __device__ __forceinline__ void load16_sc1_batch(f32x4 (&t)[N], unsigned voff, const char *const (&b)[N])
{
    if constexpr (K < N) {
        // (the load reads a COPY of its scalar base made by the scalar ALU inside the statement: the base may just have been restored from a spill lane, and a VALU
        //  write of an SGPR needs five wait states before a VMEM instruction reads it as its address -- the hazard recogniser does not look inside an asm statement,
        //  and without protection the load went off a stale base and faulted; VALU -> SALU is interlocked, SALU -> VMEM needs nothing: w2xc_device.h)
        unsigned long long bc;
        asm volatile("s_mov_b64 %1, %3\n\tglobal_load_dwordx4 %0, %2, %1 sc1" : "=v"(t[K]), "=&s"(bc) : "v"(voff), "s"(b[K]) : "memory");
        load16_sc1_batch<K + 1, N>(t, voff, b);
    }
}
template <int K, int N>
static __device__ __forceinline__ void pin_batch(f32x4 (&t)[N])
{
    if constexpr (K < N) {
        asm volatile("" : "+v"(t[K]));
        pin_batch<K + 1, N>(t);
    }
}
template <int K, int N>
static __device__ __forceinline__ void sum_batch(f32x4 &v, const f32x4 (&t)[N])
{
    if constexpr (K < N) {
        v += t[K];
        sum_batch<K + 1, N>(v, t);
    }
}

// One gather job of a PROG launch (below): the last layer's outputs of job (jr, jg) -- rows [16 jr - wino_py - g_off, + 16) x columns [256 jg, + 256) clipped to its
// plane --: out(y, x) = leaky(bias + sum over taps and 64-plane blocks of G[block][tap][y + g_off + ty][x + tx]), summed in conv3x3_last_gather_x4's order (taps outer,
// blocks inner: the two paths are bit-identical).  The other workgroups' tap planes were written through (sc1) and drained before their arrivals were counted: they
// are read with sc1 loads (past this CU's L1), no fence.  Two pixel quads per thread = 36 (NOB = 2) 16-byte loads in flight, issued as one asm batch and waited for once:
// left to the compiler -- which schedules for registers in this kernel -- every load was followed by its own vmcnt(0) (365 us per job instead of ~5).
// A FUNCTION OF ITS OWN, never inlined: as a lambda inside the kernel this code cost layer 6 0.2 ms without ever running (profiles/r6_sweeps.log 1d) -- its scalar
// state competed with the stage loop's for SGPRs and the epilogue came out differently; behind a call it has its own registers.
struct W4ProgJob {
    const float *G; long long ts, gs, rs;          // partial tap planes G[block][tap][y][x]: block / tap-plane / row strides in floats
    float *out; long long out_rs;                  // the last layer's output rows
    const float *bias;
    unsigned *flags; unsigned epoch;               // host pipeline: one word per job, written behind the rows (NULL: none)
    int g_h, g_w, g_off, wino_py, ngroups;
};
template <int NOB>
static __device__ __attribute__((noinline)) void w4_prog_job(W4ProgJob a, int jr, int jg)
{
    constexpr int ROWS = 16, GW = 8;
    auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };   // (arguments of a device function arrive in VGPRs: everything wave-uniform is made provably so)
    auto uni64 = [&](unsigned long long v) { return ((unsigned long long)(unsigned)uni((int)(unsigned)(v >> 32)) << 32) | (unsigned)uni((int)(unsigned)v); };
    jr = uni(jr); jg = uni(jg);
    const int g_h = uni(a.g_h), g_w = uni(a.g_w), g_off = uni(a.g_off);
    const long long rs = (long long)uni64((unsigned long long)a.rs), gs = (long long)uni64((unsigned long long)a.gs), ts = (long long)uni64((unsigned long long)a.ts);
    const long long out_rs = (long long)uni64((unsigned long long)a.out_rs);
    const float *G = reinterpret_cast<const float *>(uni64((unsigned long long)a.G));
    float *outp = reinterpret_cast<float *>(uni64((unsigned long long)a.out));
    const int tid = (int)threadIdx.x;
    const int y_first = ROWS * jr - uni(a.wino_py) - g_off;
    const int y_lo = y_first > 0 ? y_first : 0, y_hi = y_first + ROWS < g_h ? y_first + ROWS : g_h;
    const int x_lo = jg * GW * 32, x_hi = (jg + 1) * GW * 32 < g_w ? (jg + 1) * GW * 32 : g_w;
    const int nq = x_hi > x_lo ? (x_hi - x_lo + 3) >> 2 : 0;
    const int total = y_hi > y_lo ? (y_hi - y_lo) * nq : 0;   // (jobs of tile rows / groups outside the last layer's plane: nothing to sum, still reported)
    const float b = reinterpret_cast<const float *>(uni64((unsigned long long)a.bias))[0];
    // scalar bases of the 9 NOB (tap, block) planes, the tap's row and column shift included
    const char *gb[9 * NOB];
#pragma unroll
    for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int hf = 0; hf < NOB; hf++) gb[tap * NOB + hf] = reinterpret_cast<const char *>(uni64((unsigned long long)(G + hf * ts + tap * gs + (long long)(tap / 3) * rs + (tap % 3))));
    for (int q0 = tid; q0 < total; q0 += 1024) {
        f32x4 t0[9 * NOB], t1[9 * NOB];
        // quad q -> (row, first column); a ragged last quad of a row is loaded from the row's last four columns instead (still inside the row: it has two
        // more) and picked apart below.  32-bit byte offsets inside a tap plane (the launcher checks the plane's size).
        const bool on1 = q0 + 512 < total;
        const int qa = q0, qb = on1 ? q0 + 512 : q0;
        const int ya = qa / nq, yb = qb / nq;
        const int yy0 = y_lo + ya, yy1 = y_lo + yb, xx0 = x_lo + (qa - ya * nq) * 4, xx1 = x_lo + (qb - yb * nq) * 4;
        const bool whole0 = xx0 + 4 <= g_w, whole1 = xx1 + 4 <= g_w;
        const unsigned voff0 = (unsigned)(((long long)(yy0 + g_off) * rs + (whole0 ? xx0 : g_w - 4)) * 4);
        const unsigned voff1 = (unsigned)(((long long)(yy1 + g_off) * rs + (whole1 ? xx1 : g_w - 4)) * 4);
        load16_sc1_batch<0, 9 * NOB>(t0, voff0, gb);
        if (on1) load16_sc1_batch<0, 9 * NOB>(t1, voff1, gb);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // one wait for the batch
        pin_batch<0, 9 * NOB>(t0);
        pin_batch<0, 9 * NOB>(t1);
        auto finish = [&](bool on, const f32x4 (&t)[9 * NOB], int yy, int xx, bool whole) {
            if (!on) return;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            sum_batch<0, 9 * NOB>(v, t);
            float *oq = outp + (long long)yy * out_rs + xx;
            if (whole) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; e++) o[e] = leaky(v[e] + b);
                store16_sys(oq, o);
            } else {
                // the row's last 1..3 pixels: the batch held columns g_w - 4 .. g_w - 1 (+ the tap's shift); pixel xx + e sits at index xx + e - (g_w - 4)
                const int sh = xx - (g_w - 4);
                for (int e = 0; xx + e < g_w; e++) {
                    const int idx = sh + e;
                    const float ve = idx == 0 ? v[0] : idx == 1 ? v[1] : idx == 2 ? v[2] : v[3];
                    store4_sys(oq + e, leaky(ve + b));
                }
            }
        };
        finish(true, t0, yy0, xx0, whole0);
        finish(on1, t1, yy1, xx1, whole1);
    }
    // flags (host pipeline): the job's rows are on their way to host memory (`out` is page-locked host memory there: the stores are posted PCIe writes, issued at
    // system scope): every wave waits for its stores to have left, then ONE system-scope store publishes the job to the drainer thread, behind the data on the same link
    unsigned *flags = reinterpret_cast<unsigned *>(uni64((unsigned long long)a.flags));
    if (flags) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (tid == 0) __hip_atomic_store(flags + (jr * uni(a.ngroups) + jg), (unsigned)uni((int)a.epoch), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// PROG (with FUSE7): the launch FINISHES the fused last layer itself and finishes it in row order, so that the output plane completes top to bottom
// while the launch is still running (round 6; convertRoutine.cpp:143-161's stitch no longer waits for the layer's end):
//   * schedule: XCD k owns the tile columns [(k tiles_x + phi) / 8, ((k + 1) tiles_x + phi) / 8) of tile row r, phi = r & 7, and walks them row by row --
//     all eight XCDs work on the same tile rows at the same time (the strip walk above finishes the lower 40 % of every strip only at the very end);
//     the band edges move by at most one tile from row to row and eight rows hold exactly tiles_x tiles of every XCD: equal shares for any width;
//   * every item writes its partial tap planes through to memory (sc1) and, one item later -- when the stores have long drained --, counts its
//     arrival on the GATHER JOBS it feeds: job (r, g) = the last layer's outputs whose first tap row lies in tile row r and whose columns lie in the
//     tile group [8 g, 8 g + 8); it needs the tiles of rows r, r + 1 and columns 8 g .. 8 g + 8 (two more tap rows below, two more columns to the right);
//   * the workgroup whose arrival completes a job runs it: conv3x3_last_gather's sum (taps outer, 64-plane blocks inner: bit-identical), bias,
//     LeakyReLU, stores into the output plane; with d.prog_flags the job's completion is published to the host (system scope) for the drainer.
//   No workgroup ever waits for another one (no spinning, no residency assumption): arrivals are returning atomics, the last one does the work.
template <int CIN, int COUT, bool OUT_PLANAR, bool IN_NHWC = false, bool FUSE7 = false, bool PROG = false>
__global__ void __launch_bounds__(512, 2) conv3x3_wino4(W2xcConvDesc d, int tiles_x, int nitems)
{
#define W4B_ONLY(...)
#define W4B_SEL(b_, s_) s_
#define W4B_OUT d.out
#include "w2xc_wino4_body.inc"
#undef W4B_OUT
#undef W4B_SEL
#undef W4B_ONLY
}

// batch form (w2xc_convert_batch*): planar planes in, planar planes (FUSE7: the tap planes of the fused last layer) out, bd.batch images of bd.items items
template <int CIN, int COUT, bool FUSE7>
__global__ void __launch_bounds__(512, 2) conv3x3_wino4_batch(W2xcConvDesc d, int tiles_x, int nitems, W2xcBatchDesc bd)
{
    constexpr bool OUT_PLANAR = true, IN_NHWC = false, PROG = false;
#define W4B_ONLY(...) __VA_ARGS__
#define W4B_SEL(b_, s_) b_
#define W4B_OUT (d.out + (long long)(item / bd.items) * bd.out_bs)
#include "w2xc_wino4_body.inc"
#undef W4B_OUT
#undef W4B_SEL
#undef W4B_ONLY
}

// batch form of the multi-plane (RGB) chains: the layouts conv3x3_wino4_batch above does not have -- 32 NHWC planes in (IN_NHWC: the layer behind conv3x3_first /
// conv3x3_wino) and / or NHWC out (the layer in front of conv3x3_last); no fused last layer
template <int CIN, int COUT, bool OUT_PLANAR, bool IN_NHWC>
__global__ void __launch_bounds__(512, 2) conv3x3_wino4_batch_l(W2xcConvDesc d, int tiles_x, int nitems, W2xcBatchDesc bd)
{
    constexpr bool FUSE7 = false, PROG = false;
#define W4B_ONLY(...) __VA_ARGS__
#define W4B_SEL(b_, s_) b_
#define W4B_OUT (d.out + (long long)(item / bd.items) * bd.out_bs)
#include "w2xc_wino4_body.inc"
#undef W4B_OUT
#undef W4B_SEL
#undef W4B_ONLY
}

// ------------------------------------------------------------------------------------------------
// host side: launch (shape predicates, PROG's job arithmetic and the packers: w2xc_pack.cpp).
// Eight objects (make -j): W2XC_WINO4_PART = 0 the planar-out instantiations + dispatcher, 1 the NHWC-out ones, 2 the fused-last ones,
// 3 the batch forms with planar out + the batch dispatcher, 4 the fused-last batch forms, 5 the batch forms with 32 NHWC planes in, 6 those with planar
// planes in and NHWC out, 7 the 128 -> 256 layer of upconv models (NHWC out), 8 its batch form.
// ------------------------------------------------------------------------------------------------
#ifndef W2XC_WINO4_PART
#define W2XC_WINO4_PART -1   // one translation unit with everything (tools/ubench)
#endif
template <int CIN, int COUT, bool OUT_PLANAR, bool IN_NHWC = false, bool FUSE7 = false, bool PROG = false>
static hipError_t launch_wino4(const W2xcConvDesc &d, hipStream_t stream)
{
    const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + (d.wino_py & 3) + 15) / 16;
    const long long items = (long long)tiles_x * tiles_y * (COUT / 64);
    if (items >= (1ll << 31)) return hipErrorInvalidValue;   // (the kernel walks items in int; plan_rows caps a band below this)
    const int nitems = (int)items;
    constexpr size_t lds_bytes = 3 * (size_t)(11 * 1024) + 2 * (size_t)(36 * 1024) + 3 * (size_t)(18 * 1024) + COUT * 4 + (PROG ? 16 : 0);   // raw + U + V + bias (+ the job word)
    static_assert(lds_bytes <= 160 * 1024, "LDS budget");
    if constexpr (PROG) {
        // the job counters start at zero in EVERY launch (a memset node in front of the kernel, on its stream)
        if (!d.prog_cnt || !d.g_out || !d.g_bias || d.g_w < 4 || (long long)d.out_h * d.out_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;   // (32-bit offsets inside a tap plane, whole quads)
        hipError_t em = hipMemsetAsync(d.prog_cnt, 0, w2xc_wino4_prog_counters(d.out_w, d.out_h, d.wino_py) * sizeof(unsigned), stream);
        if (em != hipSuccess) return em;
    }
    auto kern = conv3x3_wino4<CIN, COUT, OUT_PLANAR, IN_NHWC, FUSE7, PROG>;
    static W2xcLdsOptIn opt_in;   // per (kernel, device)
    const hipError_t e = opt_in(kern, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(w2xc_persistent_grid(nitems)), dim3(512), lds_bytes, stream, d, tiles_x, nitems);
    return hipGetLastError();
}


hipError_t w2xc_launch_wino4_nhwc_out(const W2xcConvDesc &d, hipStream_t stream);
#if W2XC_WINO4_PART == 1 || W2XC_WINO4_PART == -1
hipError_t w2xc_launch_wino4_nhwc_out(const W2xcConvDesc &d, hipStream_t stream)
{
#ifdef W4P_SINGLE
    return hipErrorInvalidValue;
#else
    if (d.cin == 32 && d.in_ps == 32 && d.in_cs == 1)
        return d.cout == 64 ? launch_wino4<32, 64, false, true>(d, stream) : d.cout == 128 ? launch_wino4<32, 128, false, true>(d, stream) : hipErrorInvalidValue;
    switch (d.cin * 1000 + d.cout) {
    case 32064:  return launch_wino4<32, 64, false>(d, stream);
    case 32128:  return launch_wino4<32, 128, false>(d, stream);
    case 64064:  return launch_wino4<64, 64, false>(d, stream);
    case 64128:  return launch_wino4<64, 128, false>(d, stream);
    case 128064: return launch_wino4<128, 64, false>(d, stream);
    case 128128: return launch_wino4<128, 128, false>(d, stream);
    case 128256: return w2xc_launch_wino4_wide(d, stream);   // (part 7)
    default: return hipErrorInvalidValue;
    }
#endif
}
#endif

// 128 -> 256 planes, planar in, NHWC out: the layer in front of an upconv head.  The plain instantiation -- the item walk is tiles x (COUT / 64) for any COUT,
// and its LDS comes to exactly 160 KiB (the bias is the only term that grows); reached through w2xc_launch_wino4's checks and the NHWC-out dispatcher above
#if W2XC_WINO4_PART == 7 || W2XC_WINO4_PART == -1
hipError_t w2xc_launch_wino4_wide(const W2xcConvDesc &d, hipStream_t stream)
{
    if (d.cin != 128 || d.cout != 256 || d.in_ps != 1 || d.out_ps != 256 || d.out_cs != 1 || d.out_terms == 9) return hipErrorInvalidValue;
    return launch_wino4<128, 256, false>(d, stream);
}
#endif

// d.out_terms = 9: the one-plane last layer in the epilogue; `out` = partial tap planes G[64-plane block][tap][y][x] (out_ts / out_gs / out_rs),
// d.w7pk = the w2xc_wino4_pack_last image of its weights; W2XC_K_LAST_GATHER finishes with halves = cout / 64
hipError_t w2xc_launch_wino4_fused(const W2xcConvDesc &d, hipStream_t stream);
#if W2XC_WINO4_PART == 2 || W2XC_WINO4_PART == -1
hipError_t w2xc_launch_wino4_fused(const W2xcConvDesc &d, hipStream_t stream)
{
#ifdef W4P_SINGLE
    if (d.prog_cnt) return d.cin == 128 && d.cout == 128 && d.in_ps == 1 ? launch_wino4<128, 128, true, false, true, true>(d, stream) : hipErrorInvalidValue;
    return d.cin == 128 && d.cout == 128 && d.in_ps == 1 ? launch_wino4<128, 128, true, false, true>(d, stream) : hipErrorInvalidValue;
#else
    if (d.prog_cnt) {   // the launch finishes the last layer itself (PROG); planar 64 / 128-plane inputs (the 7-layer models' layer n - 1)
        if (d.in_ps != 1) return hipErrorInvalidValue;
        switch (d.cin * 1000 + d.cout) {
        case 64064:  return launch_wino4<64, 64, true, false, true, true>(d, stream);
        case 64128:  return launch_wino4<64, 128, true, false, true, true>(d, stream);
        case 128064: return launch_wino4<128, 64, true, false, true, true>(d, stream);
        case 128128: return launch_wino4<128, 128, true, false, true, true>(d, stream);
        default: return hipErrorInvalidValue;
        }
    }
    if (d.cin == 32 && d.in_ps == 32 && d.in_cs == 1)
        return d.cout == 64 ? launch_wino4<32, 64, true, true, true>(d, stream) : d.cout == 128 ? launch_wino4<32, 128, true, true, true>(d, stream) : hipErrorInvalidValue;
    switch (d.cin * 1000 + d.cout) {
    case 64064:  return launch_wino4<64, 64, true, false, true>(d, stream);
    case 64128:  return launch_wino4<64, 128, true, false, true>(d, stream);
    case 128064: return launch_wino4<128, 64, true, false, true>(d, stream);
    case 128128: return launch_wino4<128, 128, true, false, true>(d, stream);
    default: return hipErrorInvalidValue;
    }
#endif
}
#endif

#if W2XC_WINO4_PART == 0 || W2XC_WINO4_PART == -1
// d.wpk = w2xc_wino4_pack image; planar fp32 in (in_ps = 1, in_cs = plane stride), planar (out_ps = 1) or NHWC (out_cs = 1, out_ps = cout) out;
// d.wino_py = first output row mod 4; off_x a multiple of 4 (the engine's layers: 0)
hipError_t w2xc_launch_wino4(const W2xcConvDesc &d, hipStream_t stream)
{
    if (d.out_w <= 0 || d.out_h <= 0) return hipSuccess;
    const bool in_nhwc = d.cin == 32 && d.in_ps == 32 && d.in_cs == 1;   // the 32-plane layers in front write NHWC
    if (d.in_shift != 0 || (d.in_rs & 3) != 0 || (((size_t)d.in) & 15) != 0) return hipErrorInvalidValue;
    if (in_nhwc) {
        if (24 * d.in_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;
    } else {
        if (d.in_ps != 1 || (d.in_cs & 3) != 0 || d.off_x < 0 || (d.off_x & 3) != 0 || d.in_rs < ((d.in_w + 3) & ~3)) return hipErrorInvalidValue;
        if (3 * d.in_cs * 4 + 24 * d.in_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;   // 32-bit lane offsets inside a 4-channel slice of a tile
    }
    if (d.out_terms == 9) {   // fused last layer: partial tap planes, rows of out_w floats
        if (d.cout != 64 && d.cout != 128) return hipErrorInvalidValue;
        if (!d.w7pk || d.out_rs < d.out_w || d.out_gs < d.out_rs * (long long)d.out_h) return hipErrorInvalidValue;
        return w2xc_launch_wino4_fused(d, stream);
    }
    const bool planar = d.out_ps == 1;
    if (planar) {
        if ((d.out_rs & 3) != 0 || (d.out_cs & 3) != 0 || (((size_t)d.out) & 15) != 0 || d.out_rs < ((d.out_w + 3) & ~3)) return hipErrorInvalidValue;
    } else if (d.out_ps != d.cout || d.out_cs != 1 || (d.out_rs & 3) != 0 || (((size_t)d.out) & 15) != 0) return hipErrorInvalidValue;
    if (!planar) return w2xc_launch_wino4_nhwc_out(d, stream);
#ifndef W4P_SINGLE
    if (in_nhwc) return d.cout == 64 ? launch_wino4<32, 64, true, true>(d, stream) : d.cout == 128 ? launch_wino4<32, 128, true, true>(d, stream) : hipErrorInvalidValue;
#endif
#ifdef W4P_SINGLE   // (development builds: one instantiation)
    return d.cin == 128 && d.cout == 128 ? launch_wino4<128, 128, true>(d, stream) : hipErrorInvalidValue;
#else
    switch (d.cin * 1000 + d.cout) {
    case 32064:  return launch_wino4<32, 64, true>(d, stream);
    case 32128:  return launch_wino4<32, 128, true>(d, stream);
    case 64064:  return launch_wino4<64, 64, true>(d, stream);
    case 64128:  return launch_wino4<64, 128, true>(d, stream);
    case 128064: return launch_wino4<128, 64, true>(d, stream);
    case 128128: return launch_wino4<128, 128, true>(d, stream);
    default: return hipErrorInvalidValue;
    }
#endif
}
#endif

// ---- batch forms (w2xc_convert_batch*): the single-image launch of every image at once ----
template <int CIN, int COUT, bool FUSE7>
static hipError_t launch_wino4_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + (d.wino_py & 3) + 15) / 16;
    const long long items = (long long)tiles_x * tiles_y * (COUT / 64);
    if (items * b.batch >= (1ll << 31)) return hipErrorInvalidValue;
    b.items = (int)items;
    const int nitems = (int)(items * b.batch);
    constexpr size_t lds_bytes = 3 * (size_t)(11 * 1024) + 2 * (size_t)(36 * 1024) + 3 * (size_t)(18 * 1024) + COUT * 4;   // raw + U + V + bias
    static_assert(lds_bytes <= 160 * 1024, "LDS budget");
    auto kern = conv3x3_wino4_batch<CIN, COUT, FUSE7>;
    static W2xcLdsOptIn opt_in;   // per (kernel, device)
    const hipError_t e = opt_in(kern, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(w2xc_persistent_grid(nitems)), dim3(512), lds_bytes, stream, d, tiles_x, nitems, b);
    return hipGetLastError();
}

template <int CIN, int COUT, bool OUT_PLANAR, bool IN_NHWC>
static hipError_t launch_wino4_batch_l(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + (d.wino_py & 3) + 15) / 16;
    const long long items = (long long)tiles_x * tiles_y * (COUT / 64);
    if (items * b.batch >= (1ll << 31)) return hipErrorInvalidValue;
    b.items = (int)items;
    const int nitems = (int)(items * b.batch);
    constexpr size_t lds_bytes = 3 * (size_t)(11 * 1024) + 2 * (size_t)(36 * 1024) + 3 * (size_t)(18 * 1024) + COUT * 4;   // raw + U + V + bias
    static_assert(lds_bytes <= 160 * 1024, "LDS budget");
    auto kern = conv3x3_wino4_batch_l<CIN, COUT, OUT_PLANAR, IN_NHWC>;
    static W2xcLdsOptIn opt_in;   // per (kernel, device)
    const hipError_t e = opt_in(kern, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(w2xc_persistent_grid(nitems)), dim3(512), lds_bytes, stream, d, tiles_x, nitems, b);
    return hipGetLastError();
}

// 32 NHWC planes in, planar or NHWC out (d.out_ps tells); the dispatcher below has checked everything but the output layout's alignment
hipError_t w2xc_launch_wino4_batch_nhwc_in(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream);
#if W2XC_WINO4_PART == 5 || W2XC_WINO4_PART == -1
hipError_t w2xc_launch_wino4_batch_nhwc_in(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    if (d.out_ps == 1) return d.cout == 64 ? launch_wino4_batch_l<32, 64, true, true>(d, b, stream) : d.cout == 128 ? launch_wino4_batch_l<32, 128, true, true>(d, b, stream) : hipErrorInvalidValue;
    return d.cout == 64 ? launch_wino4_batch_l<32, 64, false, true>(d, b, stream) : d.cout == 128 ? launch_wino4_batch_l<32, 128, false, true>(d, b, stream) : hipErrorInvalidValue;
}
#endif

// planar planes in (64 / 128 of them), NHWC out
hipError_t w2xc_launch_wino4_batch_nhwc_out(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream);
#if W2XC_WINO4_PART == 6 || W2XC_WINO4_PART == -1
hipError_t w2xc_launch_wino4_batch_nhwc_out(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    switch (d.cin * 1000 + d.cout) {
    case 64064:  return launch_wino4_batch_l<64, 64, false, false>(d, b, stream);
    case 64128:  return launch_wino4_batch_l<64, 128, false, false>(d, b, stream);
    case 128064: return launch_wino4_batch_l<128, 64, false, false>(d, b, stream);
    case 128128: return launch_wino4_batch_l<128, 128, false, false>(d, b, stream);
    default: return hipErrorInvalidValue;
    }
}
#endif

// 128 -> 256 planes, planar in, NHWC out: the batch form of the layer in front of an upconv head (w2xc_launch_wino4_wide): one more instantiation of the
// batch body, 160 KiB of LDS like the one-image launch
hipError_t w2xc_launch_wino4_batch_wide(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream);
#if W2XC_WINO4_PART == 8 || W2XC_WINO4_PART == -1
hipError_t w2xc_launch_wino4_batch_wide(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    if (d.cin != 128 || d.cout != 256 || d.in_ps != 1 || d.out_ps != 256 || d.out_cs != 1 || d.out_terms == 9) return hipErrorInvalidValue;
    return launch_wino4_batch_l<128, 256, false, false>(d, b, stream);
}
#endif

hipError_t w2xc_launch_wino4_batch_fused(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream);
#if W2XC_WINO4_PART == 4 || W2XC_WINO4_PART == -1
hipError_t w2xc_launch_wino4_batch_fused(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    switch (d.cin * 1000 + d.cout) {
    case 64064:  return launch_wino4_batch<64, 64, true>(d, b, stream);
    case 64128:  return launch_wino4_batch<64, 128, true>(d, b, stream);
    case 128064: return launch_wino4_batch<128, 64, true>(d, b, stream);
    case 128128: return launch_wino4_batch<128, 128, true>(d, b, stream);
    default: return hipErrorInvalidValue;
    }
}
#endif

#if W2XC_WINO4_PART == 3 || W2XC_WINO4_PART == -1
// d = the single-image descriptor (the checks of w2xc_launch_wino4 apply to it unchanged), b.in_bs / b.out_bs = image strides in floats (multiples of 4:
// every image's planes keep the 16-byte alignment of image 0's)
hipError_t w2xc_launch_wino4_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    if (d.out_w <= 0 || d.out_h <= 0 || b.batch == 0) return hipSuccess;
    if (b.batch < 0 || b.in_bs < 0 || b.out_bs < 0 || (b.in_bs & 3) != 0 || (b.out_bs & 3) != 0) return hipErrorInvalidValue;
    if (d.in_shift != 0 || (d.in_rs & 3) != 0 || (((size_t)d.in) & 15) != 0 || d.prog_cnt) return hipErrorInvalidValue;
    const bool in_nhwc = d.cin == 32 && d.in_ps == 32 && d.in_cs == 1, out_nhwc = d.out_terms != 9 && d.out_ps != 1;
    if (in_nhwc || out_nhwc) {   // the layouts of the multi-plane chains (w2xc_wino4_batch_layout_supported); the checks of w2xc_launch_wino4
        if (!w2xc_wino4_batch_layout_supported(d.cin, d.cout, in_nhwc, !out_nhwc) || d.out_terms == 9) return hipErrorInvalidValue;
        if (in_nhwc) {
            if (24 * d.in_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;
        } else {
            if (d.in_ps != 1 || (d.in_cs & 3) != 0 || d.off_x < 0 || (d.off_x & 3) != 0 || d.in_rs < ((d.in_w + 3) & ~3)) return hipErrorInvalidValue;
            if (3 * d.in_cs * 4 + 24 * d.in_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;
        }
        if (out_nhwc) {
            if (d.out_ps != d.cout || d.out_cs != 1 || (d.out_rs & 3) != 0 || (((size_t)d.out) & 15) != 0) return hipErrorInvalidValue;
        } else if ((d.out_rs & 3) != 0 || (d.out_cs & 3) != 0 || (((size_t)d.out) & 15) != 0 || d.out_rs < ((d.out_w + 3) & ~3)) return hipErrorInvalidValue;
        if (!in_nhwc && d.cout == 256) return w2xc_launch_wino4_batch_wide(d, b, stream);   // (part 8)
        return in_nhwc ? w2xc_launch_wino4_batch_nhwc_in(d, b, stream) : w2xc_launch_wino4_batch_nhwc_out(d, b, stream);
    }
    if (d.in_ps != 1 || (d.in_cs & 3) != 0 || d.off_x < 0 || (d.off_x & 3) != 0 || d.in_rs < ((d.in_w + 3) & ~3)) return hipErrorInvalidValue;
    if (3 * d.in_cs * 4 + 24 * d.in_rs * 4 >= (1ll << 32)) return hipErrorInvalidValue;   // 32-bit lane offsets inside a 4-channel slice of a tile
    if (!w2xc_wino4_batch_supported(d.cin, d.cout, d.out_terms == 9)) return hipErrorInvalidValue;
    if (d.out_terms == 9) {   // fused last layer: partial tap planes, rows of out_w floats
        if (!d.w7pk || d.out_rs < d.out_w || d.out_gs < d.out_rs * (long long)d.out_h) return hipErrorInvalidValue;
        return w2xc_launch_wino4_batch_fused(d, b, stream);
    }
    if (d.out_ps != 1 || (d.out_rs & 3) != 0 || (d.out_cs & 3) != 0 || (((size_t)d.out) & 15) != 0 || d.out_rs < ((d.out_w + 3) & ~3)) return hipErrorInvalidValue;
    switch (d.cin * 1000 + d.cout) {
    case 32064:  return launch_wino4_batch<32, 64, false>(d, b, stream);
    case 32128:  return launch_wino4_batch<32, 128, false>(d, b, stream);
    case 64064:  return launch_wino4_batch<64, 64, false>(d, b, stream);
    case 64128:  return launch_wino4_batch<64, 128, false>(d, b, stream);
    case 128064: return launch_wino4_batch<128, 64, false>(d, b, stream);
    case 128128: return launch_wino4_batch<128, 128, false>(d, b, stream);
    default: return hipErrorInvalidValue;
    }
}
#endif
