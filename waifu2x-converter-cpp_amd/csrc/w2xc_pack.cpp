// w2xc_pack.cpp -- kernel selection by layer shape and every weight packer of the library (see w2xc_pack.hpp): loops over floats on the host, no HIP.
// Each packer's comment states the address of weight W[o][c][tap] in its image; the kernel named there reads exactly that order.
#include "w2xc_pack.hpp"
#include "w2xc_layout.h"

#include <math.h>
#include <stdint.h>
#include <string.h>

static bool is_mid(int c) { return c == 32 || c == 64 || c == 128; }

W2xcKernelKind w2xc_pick_kernel(int cin, int cout)
{
    if (is_mid(cin) && is_mid(cout)) return W2XC_K_MFMA;
    if ((cin == 1 || cin == 3) && is_mid(cout)) return W2XC_K_FIRST;
    if (is_mid(cin) && (cout == 1 || cout == 3)) return W2XC_K_LAST;
    return W2XC_K_DIRECT;
}

const char *w2xc_kernel_name(W2xcKernelKind kind, int cin, int cout)
{
    (void)cin; (void)cout;
    switch (kind) {
    case W2XC_K_MFMA: return "conv3x3_mfma";
    case W2XC_K_FIRST: return "conv3x3_first";
    case W2XC_K_LAST: return "conv3x3_last";
    case W2XC_K_MID_SPLIT: return "conv3x3_split";
    case W2XC_K_FIRST_SPLIT: return "conv3x3_first_split";
    case W2XC_K_LAST_GATHER: return "conv3x3_last_gather";
    case W2XC_K_FIRST2_SPLIT: return "conv3x3_first2_split";
    case W2XC_K_FUSED_AWAY: return "(in_next_layer)";
    case W2XC_K_FIRST2_WINO4: return "conv3x3_first2_wino4";
    case W2XC_K_FIRST_U8: return "conv3x3_first_u8";
    case W2XC_K_LAST_U8: return "conv3x3_last_u8";
    case W2XC_K_UPCONV: return "upconv4x4_head";
    case W2XC_K_UPCONV_U8: return "upconv4x4_head_u8";
    case W2XC_K_UPCONV_A_U8: return "upconv4x4_head_alpha_u8";
    case W2XC_K_UPCONV_A: return "upconv4x4_head_alpha";
    default: return "conv3x3_direct";
    }
}

// ------------------------------------------------------------------------------------------------
// fp32 kernels of w2xc_kernels.hip
// ------------------------------------------------------------------------------------------------
size_t w2xc_packed_weight_floats(W2xcKernelKind kind, int cin, int cout)
{
    switch (kind) {
    case W2XC_K_MFMA: return (size_t)9 * cin * cout;
    case W2XC_K_FIRST: case W2XC_K_FIRST_SPLIT: return (size_t)(cout / 32) * ((9 * cin + 1) / 2) * W2XC_WAVE;
    case W2XC_K_LAST: return (size_t)(cin / 16) * 4 * ((9 * cout + 15) / 16) * W2XC_WAVE;
    default: return (size_t)cin * 9 * direct_cout_pad(cout);
    }
}

// W2XC_K_MFMA   (conv3x3_mfma2): wpk[tap][c / 8][nb][lane][j] = W[32 nb + (lane & 31)][8 (c / 8) + 4 (lane >> 5) + j][tap]
// W2XC_K_FIRST  (conv3x3_first, conv3x3_first_split): wpk[nb][s][lane] = W[32 nb + (lane & 31)][k / 9][k % 9], k = 2 s + (lane >> 5); 0 for k >= K = 9 cin
// W2XC_K_LAST   (conv3x3_last): wpk[c / 16][j][nb][lane] = W[n % cout][16 (c / 16) + 4 (lane >> 4) + j][n / cout], n = 16 nb + (lane & 15); 0 for n >= 9 cout
// W2XC_K_DIRECT (conv3x3_direct): wpk[c][tap][o], rows of cout padded to DIRECT_CG; 0 for o >= cout
void w2xc_pack_weights(W2xcKernelKind kind, int cin, int cout, const float *w, float *dst)
{
    auto W = [&](int o, int i, int tap) { return w[((size_t)o * cin + i) * 9 + tap]; };
    memset(dst, 0, w2xc_packed_weight_floats(kind, cin, cout) * sizeof(float));
    if (kind == W2XC_K_FIRST_SPLIT) kind = W2XC_K_FIRST;
    if (kind == W2XC_K_MFMA) {
        const int nbt = cout / 32, c8n = cin / 8;
        for (int tap = 0; tap < 9; tap++)
            for (int c8 = 0; c8 < c8n; c8++)
                for (int nb = 0; nb < nbt; nb++)
                    for (int lane = 0; lane < W2XC_WAVE; lane++)
                        for (int j = 0; j < 4; j++) {
                            const int kk = lane >> 5, n = lane & 31;
                            dst[((((size_t)tap * c8n + c8) * nbt + nb) * W2XC_WAVE + lane) * 4 + j] =
                                W(nb * 32 + n, c8 * 8 + kk * 4 + j, tap);
                        }
    } else if (kind == W2XC_K_FIRST) {
        const int nbt = cout / 32, K = 9 * cin, S = (K + 1) / 2;
        for (int nb = 0; nb < nbt; nb++)
            for (int s = 0; s < S; s++)
                for (int lane = 0; lane < W2XC_WAVE; lane++) {
                    const int k = 2 * s + (lane >> 5);
                    dst[((size_t)nb * S + s) * W2XC_WAVE + lane] = k < K ? W(nb * 32 + (lane & 31), k / 9, k % 9) : 0.0f;
                }
    } else if (kind == W2XC_K_LAST) {
        const int N = 9 * cout, nb16 = (N + 15) / 16, s4n = cin / 16;
        for (int s4 = 0; s4 < s4n; s4++)
            for (int j = 0; j < 4; j++)
                for (int nb = 0; nb < nb16; nb++)
                    for (int lane = 0; lane < W2XC_WAVE; lane++) {
                        const int n = nb * 16 + (lane & 15), c = 16 * s4 + 4 * (lane >> 4) + j;
                        dst[(((size_t)s4 * 4 + j) * nb16 + nb) * W2XC_WAVE + lane] = n < N ? W(n % cout, c, n / cout) : 0.0f;
                    }
    } else {
        const int cp = direct_cout_pad(cout);
        for (int i = 0; i < cin; i++)
            for (int tap = 0; tap < 9; tap++)
                for (int o = 0; o < cout; o++) dst[((size_t)i * 9 + tap) * cp + o] = W(o, i, tap);
    }
}

// ------------------------------------------------------------------------------------------------
// upconv4x4_head (w2xc_upconv.hip): the 4x4 stride-2 transposed convolution that ends an upconv model
// ------------------------------------------------------------------------------------------------
bool w2xc_upconv_supported(int cin, int nout) { return (is_mid(cin) || cin == 256) && (nout == 1 || nout == 3); }
size_t w2xc_upconv_packed_floats(int cin, int nout) { return (size_t)16 * nout * cin; }

// wpk[c / 16][j][nb][lane] = Wt[c][n % nout][n / nout], c = 16 (c / 16) + 4 (lane >> 4) + j, n = 16 nb + (lane & 15) = tap * nout + o, tap = 4 r + s:
// conv3x3_last's "taps as N" image with 16 taps; N = 16 nout is whole 16-column blocks, so every lane of the image is a weight and every weight has one lane
void w2xc_upconv_pack(int cin, int nout, const float *w, float *dst)
{
    const int nb16 = nout, s4n = cin / 16;
    for (int s4 = 0; s4 < s4n; s4++)
        for (int j = 0; j < 4; j++)
            for (int nb = 0; nb < nb16; nb++)
                for (int lane = 0; lane < W2XC_WAVE; lane++) {
                    const int n = nb * 16 + (lane & 15), c = 16 * s4 + 4 * (lane >> 4) + j;
                    dst[(((size_t)s4 * 4 + j) * nb16 + nb) * W2XC_WAVE + lane] = w[((size_t)c * nout + n % nout) * 16 + n / nout];
                }
}

void w2xc_upconv_pack_alpha(int cin, const float *w, float *dst)
{
    // w2xc_upconv_pack(cin, 1, Wt[:, 1], dst) without the copy of the slice: plane c's 16 taps lie at w + (3 c + 1) * 16, and with one output n = tap
    for (int s4 = 0; s4 < cin / 16; s4++)
        for (int j = 0; j < 4; j++)
            for (int lane = 0; lane < W2XC_WAVE; lane++) {
                const int c = 16 * s4 + 4 * (lane >> 4) + j;
                dst[((size_t)s4 * 4 + j) * W2XC_WAVE + lane] = w[((size_t)c * 3 + 1) * 16 + (lane & 15)];
            }
}

// one workgroup per tile up to two per CU (512); beyond that every workgroup walks a run of consecutive tiles
int w2xc_upconv_grid(int ntiles) { return ntiles < 512 ? ntiles : 512; }

void w2xc_pad_layer(int cin, int cout, int cin_p, int cout_p, const float *w, float *dst)
{
    memset(dst, 0, (size_t)cin_p * cout_p * 9 * sizeof(float));
    for (int o = 0; o < cout; o++)
        for (int i = 0; i < cin; i++) memcpy(dst + ((size_t)o * cin_p + i) * 9, w + ((size_t)o * cin + i) * 9, 9 * sizeof(float));
}

void w2xc_pad_head(int cin, int nout, int cin_p, const float *w, float *dst)
{
    memset(dst, 0, (size_t)cin_p * nout * 16 * sizeof(float));
    memcpy(dst, w, (size_t)cin * nout * 16 * sizeof(float));
}

// ------------------------------------------------------------------------------------------------
// Winograd F(2x2, 3x3): conv3x3_wino
// ------------------------------------------------------------------------------------------------
bool w2xc_wino_supported(int cin, int cout) { return is_mid(cin) && is_mid(cout); }

size_t w2xc_wino_packed_floats(int cin, int cout) { return (size_t)W2XC_WINO_XI * cin * cout; }

// U = G g G^T for one 3x3 filter g and an N x 3 matrix G, formed in double (rounded once, by the caller)
template <int N>
static void filter_transform(const double (&G)[N][3], const float *g, double (&U)[N][N])
{
    double tmp[N][3];
    for (int i = 0; i < N; i++)
        for (int j = 0; j < 3; j++) tmp[i][j] = G[i][0] * g[0 * 3 + j] + G[i][1] * g[1 * 3 + j] + G[i][2] * g[2 * 3 + j];
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) U[i][j] = tmp[i][0] * G[j][0] + tmp[i][1] * G[j][1] + tmp[i][2] * G[j][2];
}

// wpk[plane block][slice][k-group G][step s][xi / 4][lane][xi % 4] = U_xi[o][c],  U = G g G^T  (G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]),
// o = 32*block + (lane & 31), c = 16*slice + 8*(lane >> 5) + 2*G + s; the products with 1/2 and 1/4 are formed in double and rounded once.
void w2xc_wino_pack(int cin, int cout, const float *w, float *dst)
{
    static const double GM[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    const int nsl = cin / 16, nob = cout / 32;
    for (int ob = 0; ob < nob; ob++)
        for (int sl = 0; sl < nsl; sl++)
            for (int G = 0; G < 4; G++)
                for (int s = 0; s < 2; s++)
                    for (int lane = 0; lane < W2XC_WAVE; lane++) {
                        const int o = 32 * ob + (lane & 31), c = 16 * sl + 8 * (lane >> 5) + 2 * G + s;
                        double U[4][4];
                        filter_transform(GM, w + ((size_t)o * cin + c) * 9, U);
                        for (int xi = 0; xi < W2XC_WINO_XI; xi++)
                            dst[((((((size_t)ob * nsl + sl) * 4 + G) * 2 + s) * 4 + (xi >> 2)) * W2XC_WAVE + lane) * 4 + (xi & 3)] = (float)U[xi >> 2][xi & 3];
                    }
}

// ------------------------------------------------------------------------------------------------
// Winograd F(4x4, 3x3): conv3x3_wino4, conv3x3_first2_wino4
// ------------------------------------------------------------------------------------------------
// G of the Cook-Toom points 0, +-3/4, +-3/2, inf (w2xc_wino4_math.h has B^T and A^T, the kernels' side)
static const double WINO4_G[6][3] = {{64.0 / 81, 0, 0},
                                     {-128.0 / 243, -32.0 / 81, -8.0 / 27},
                                     {-128.0 / 243, 32.0 / 81, -8.0 / 27},
                                     {32.0 / 243, 16.0 / 81, 8.0 / 27},
                                     {32.0 / 243, -16.0 / 81, 8.0 / 27},
                                     {0, 0, 1}};

bool w2xc_wino4_supported(int cin, int cout) { return is_mid(cin) && (cout == 64 || cout == 128); }
// PROG: the fused launch that finishes the last layer itself exists for planar 64 / 128-plane inputs
bool w2xc_wino4_prog_supported(int cin, int cout) { return (cin == 64 || cin == 128) && (cout == 64 || cout == 128); }
// planar in (in_ps = 1) only: the 32-plane NHWC-in forms and PROG have no batch instantiation (the engine's batch chain never needs them)
bool w2xc_wino4_batch_supported(int cin, int cout, bool fused_last)
{
    return fused_last ? (cin == 64 || cin == 128) && (cout == 64 || cout == 128) : w2xc_wino4_supported(cin, cout);
}
bool w2xc_wino4_batch_layout_supported(int cin, int cout, bool in_nhwc, bool out_planar)
{
    if (cin == 128 && cout == 256) return !in_nhwc && !out_planar;   // (the layer in front of an upconv head: planar in, NHWC out)
    if (cout != 64 && cout != 128) return false;
    if (in_nhwc) return cin == 32;
    return out_planar ? w2xc_wino4_batch_supported(cin, cout, false) : (cin == 64 || cin == 128);
}
bool w2xc_wino_batch_supported(int cin, int cout) { return is_mid(cin) && cout == 32; }

// ... and PROG's control words: per job (tile row, group of 8 tile columns of the launch's region) an arrival counter and a queue slot, + head and tail
void w2xc_wino4_prog_jobs(int out_w, int out_h, int wino_py, int *tile_rows, int *groups)
{
    *tile_rows = (out_h + (wino_py & 3) + 15) / 16;
    *groups = ((out_w + 31) / 32 + 7) / 8;
}
size_t w2xc_wino4_prog_counters(int out_w, int out_h, int wino_py)
{
    int tile_rows, groups;
    w2xc_wino4_prog_jobs(out_w, out_h, wino_py, &tile_rows, &groups);
    return 2 * (size_t)tile_rows * groups + 2;   // arrivals per job | the ready queue | head, tail
}

// wpk[64-plane block ob][stage s (4 channels)][xi / 4][plane tile pt][lane = 16 k + o][xi % 4] = U_xi[plane 64 ob + 16 pt + o][channel 4 s + k], xi = xi_of(i, j),
// U = G g G^T formed in double and rounded once.  36 * cin * cout floats.
void w2xc_wino4_pack(int cin, int cout, const float *w, float *dst)
{
    const int nst = cin / 4, nob = cout / 64;
    for (int ob = 0; ob < nob; ob++)
        for (int s = 0; s < nst; s++)
            for (int pt = 0; pt < 4; pt++)
                for (int k = 0; k < 4; k++)
                    for (int o = 0; o < 16; o++) {
                        const int plane = 64 * ob + 16 * pt + o, c = 4 * s + k;
                        double U[6][6];
                        filter_transform(WINO4_G, w + ((size_t)plane * cin + c) * 9, U);
                        for (int i = 0; i < 6; i++)
                            for (int j = 0; j < 6; j++) {
                                const int xi = xi_of(i, j);
                                dst[(((((size_t)ob * nst + s) * (W2XC_WINO4_XI / 4) + (xi >> 2)) * 4 + pt) * W2XC_WAVE + k * 16 + o) * 4 + (xi & 3)] = (float)U[i][j];
                            }
                    }
}

// the last layer's weights as MFMA A fragments for conv3x3_wino4's fused epilogue: [16-plane group g][e][lane = 16 kk + m] = w7[plane 16 g + 4 kk + e][tap m]
// (m < 9, else 0).  w is [1][cin][3][3].  16 * cin floats.
size_t w2xc_wino4_pack_last_floats(int cin) { return (size_t)16 * cin; }
void w2xc_wino4_pack_last(int cin, const float *w, float *dst)
{
    for (int g = 0; g < cin / 16; g++)
        for (int e = 0; e < 4; e++)
            for (int kk = 0; kk < 4; kk++)
                for (int m = 0; m < 16; m++) dst[((size_t)g * 4 + e) * W2XC_WAVE + kk * 16 + m] = m < 9 ? w[(size_t)(16 * g + 4 * kk + e) * 9 + m] : 0.0f;
}

bool w2xc_first2_wino4_supported(int cin1, int cout1, int cout2) { return cin1 == 1 && cout1 == 32 && cout2 == 32; }

// conv3x3_first2_wino4, layer 2's weights: wpk[wave g][xi - 9 g][plane tile pt][k-step ks][lane = 16 k + o] = U_xi[plane 16 pt + o][channel 4 ks + k], xi = 6 i + j,
// U = G g G^T formed in double and rounded once.  w is [32][32][3][3].  36 * 32 * 32 floats.
void w2xc_first2_wino4_pack(const float *w, float *dst)
{
    const int cin = 32, cout = 32;
    for (int plane = 0; plane < cout; plane++)
        for (int c = 0; c < cin; c++) {
            double U[6][6];
            filter_transform(WINO4_G, w + ((size_t)plane * cin + c) * 9, U);
            const int pt = plane / 16, o = plane % 16, ks = c / 4, k = c % 4;
            for (int xi = 0; xi < W2XC_WINO4_XI; xi++)
                dst[((((size_t)(xi / 9) * 9 + xi % 9) * 2 + pt) * 8 + ks) * W2XC_WAVE + k * 16 + o] = (float)U[xi / 6][xi % 6];
        }
}

// ------------------------------------------------------------------------------------------------
// split kernels (w2xc_split.hip): fp32 weights as sums of 16-bit terms
// ------------------------------------------------------------------------------------------------
// float -> bf16 / fp16 bits, round to nearest even (what v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 do), and back (exact)
static uint16_t bf16_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static float bf16_value(uint16_t h)
{
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint16_t fp16_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint32_t sign = u & 0x80000000u;
    u ^= sign;
    uint16_t h;
    if (u >= 0x47800000u) {                    // |f| >= 2^16, inf, NaN
        h = u > 0x7F800000u ? 0x7E00 : 0x7C00;
    } else if (u < 0x38800000u) {              // |f| < 2^-14: a subnormal fp16 -- adding 1/2 puts the last kept bit (2^-24) at the float's last bit, the FPU rounds
        float a;
        memcpy(&a, &u, 4);
        a += 0.5f;
        memcpy(&u, &a, 4);
        h = (uint16_t)(u - 0x3F000000u);
    } else {                                   // normal: rebias the exponent, round the 13 dropped bits to nearest even (a carry may reach the exponent: right)
        const uint32_t odd = (u >> 13) & 1u;
        u += ((uint32_t)(15 - 127) << 23) + 0xFFFu + odd;
        h = (uint16_t)(u >> 13);
    }
    return (uint16_t)(h | (sign >> 16));
}
static float fp16_value(uint16_t h)
{
    const int e = (h >> 10) & 31, m = h & 0x3FF;
    const float a = e == 31 ? (m ? NAN : INFINITY) : e ? ldexpf((float)(m | 0x400), e - 25) : ldexpf((float)m, -24);
    return (h & 0x8000) ? -a : a;
}

// r = out[0] + out[1] (+ out[2]) + a remainder: out[t] = rnd16(r - out[0] - .. - out[t - 1]), every difference exact in fp32.  fmt 0: bf16, 1: fp16
static void split_terms(float r, int terms, int fmt, uint16_t *out)
{
    for (int t = 0; t < terms; t++) {
        out[t] = fmt == 1 ? fp16_bits(r) : bf16_bits(r);
        r -= fmt == 1 ? fp16_value(out[t]) : bf16_value(out[t]);
    }
}

// fp16 terms: the power of two S that puts max|w| into [2^14, 2^15): the low term of every weight down to 2^-17 max|w| is then a NORMAL fp16
// number (22 significant bits in two terms).  1 for all-zero (or non-finite) weights.
static float fp16_weight_scale(const float *w, size_t n)
{
    float mx = 0.0f;
    for (size_t i = 0; i < n; i++) mx = fabsf(w[i]) > mx ? fabsf(w[i]) : mx;
    if (!(mx > 0.0f && mx < INFINITY)) return 1.0f;
    int e = 0;
    frexpf(mx, &e);                 // mx = f * 2^e, f in [0.5, 1)
    return ldexpf(1.0f, 15 - e);    // mx * scale in [2^14, 2^15)
}

// k-groups (16-channel layout groups) per stage: one for the two/three-term modes; the one-term mode has a third of
// the MFMAs per byte and takes 64-channel stages to amortise the stage barrier
int w2xc_split_kg(int terms, int cin) { return terms == 1 ? (cin >= 64 ? 4 : 2) : 1; }

size_t w2xc_split_packed_bytes(int cin, int cout, int terms) { return (size_t)9 * cin * cout * 2 * terms; }

// conv3x3_split, conv3x3_first2_split:
// wpk[tap][slice][term][g][nb][lane][8] (16-bit) = term `term` of S * W[32*nb + (lane&31)][slice*16*KG + 16*g + 8*(lane>>5) + e][tap]
// fmt 0: bf16 terms, S = 1.  fmt 1: fp16 terms, S = fp16_weight_scale.  Returns S; the consumer multiplies its accumulators by 1/S (exact).
float w2xc_split_pack(int cin, int cout, int terms, int fmt, const float *w, void *dst)
{
    const float scale = fmt == 1 ? fp16_weight_scale(w, (size_t)9 * cin * cout) : 1.0f;
    const int kg = w2xc_split_kg(terms, cin), nsl = cin / (16 * kg), nbt = cout / 32;
    uint16_t *d16 = static_cast<uint16_t *>(dst);
    for (int tap = 0; tap < 9; tap++)
        for (int sl = 0; sl < nsl; sl++)
            for (int nb = 0; nb < nbt; nb++)
                for (int g = 0; g < kg; g++)
                    for (int lane = 0; lane < W2XC_WAVE; lane++)
                        for (int e = 0; e < 8; e++) {
                            const int o = nb * 32 + (lane & 31), c = sl * 16 * kg + 16 * g + 8 * (lane >> 5) + e;
                            uint16_t h[3];
                            split_terms(w[((size_t)o * cin + c) * 9 + tap] * scale, terms, fmt, h);   // (the product is exact: a power of two)
                            for (int t = 0; t < terms; t++) d16[((((((size_t)tap * nsl + sl) * terms + t) * kg + g) * nbt + nb) * W2XC_WAVE + lane) * 8 + e] = h[t];
                        }
    return scale;
}

// wave columns (WN) of the tile shape that launch_split_t (w2xc_split.hip) runs a (cin, cout) layer with at `terms` terms = partial-G planes
// the fused epilogue writes (each wave column writes its own nine tap planes).  Two terms: 2 for 64 / 128 planes; one and three terms: 2 for
// 128 planes -- and for the one-term 64 -> 64 shape, which runs 8 waves of 4 rows x 32 planes (answered 1 here, the gather dropped planes
// 32..63 and the second wave column stored past the nine tap planes the workspace was sized for).
int w2xc_split_halves(int terms, int cin, int cout)
{
    if (terms == 2) return cout >= 64 ? 2 : 1;
    if (terms == 1 && cin == 64 && cout == 64) return 2;
    return cout >= 128 ? 2 : 1;
}

size_t w2xc_split_pack_last_bytes(int cin, int terms) { return (size_t)terms * (cin / 32) * 2 * W2XC_WAVE * 8 * 2; }

// conv3x3_split<.., OT = 9>: w7pk[term < terms][plane block][k-group h][lane][8] = term of S * W[0][c][tap = lane & 31] (0 for taps >= 9), with
// c = 32*block + 16*h + 4*(lane>>5) + (e < 4 ? e : 4 + e)   -- the channel order of the accumulator registers 8h .. 8h+7.
// Same scale rule as w2xc_split_pack.  w is [1][cin][3][3].
float w2xc_split_pack_last(int cin, int terms, int fmt, const float *w, void *dst)
{
    const float scale = fmt == 1 ? fp16_weight_scale(w, (size_t)9 * cin) : 1.0f;
    const int nbt = cin / 32;
    uint16_t *d16 = static_cast<uint16_t *>(dst);
    for (int nb = 0; nb < nbt; nb++)
        for (int h = 0; h < 2; h++)
            for (int lane = 0; lane < W2XC_WAVE; lane++)
                for (int e = 0; e < 8; e++) {
                    const int tap = lane & 31, kk = lane >> 5;
                    const int c = 32 * nb + 16 * h + 4 * kk + (e < 4 ? e : 4 + e);
                    uint16_t hv[3];
                    split_terms(tap < 9 ? w[(size_t)c * 9 + tap] * scale : 0.0f, terms, fmt, hv);
                    for (int t = 0; t < terms; t++) d16[((((size_t)t * nbt + nb) * 2 + h) * W2XC_WAVE + lane) * 8 + e] = hv[t];
                }
    return scale;
}
