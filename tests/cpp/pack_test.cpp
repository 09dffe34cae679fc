// pack_test.cpp -- the weight packers (waifu2x-converter-cpp_amd/csrc/w2xc_pack.cpp) checked as properties on the CPU: built with g++ from that file
// alone (no HIP, no library).  What is asserted is what the KERNELS need, from the layouts their fragment addressing documents:
//   * every weight W[o][c][tap] (Winograd: U = G g G^T of filter W[o][c]) is found at its documented address, every other slot of the image is exactly 0;
//   * the 16-bit terms of the split images add up to the weight as closely as the number formats promise (bounds derived at each check);
//   * the two F(4x4,3x3) packers hold the same U; PROG's counter count belongs to its job grid.
// Prints the first failing input of each property; exit status = number of failed properties.
#include "../../waifu2x-converter-cpp_amd/csrc/w2xc_pack.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int g_failed = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s -- ", __func__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                     \
            std::printf("\n");                                            \
            g_failed++;                                                   \
            return;                                                       \
        }                                                                 \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd32()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}
// a float with a full 24-bit significand and a binary exponent drawn from [lo, hi]: no weight shares its value with another one
static float rnd_float(int lo, int hi)
{
    const float m = (float)((rnd32() & 0x7FFFFFu) | 0x800000u) * (rnd32() & 1 ? 1.0f : -1.0f);   // 2^23 <= |m| < 2^24
    return std::ldexp(m, lo - 23 + (int)(rnd32() % (unsigned)(hi - lo + 1)));
}
static std::vector<float> weights(int cout, int cin, int lo = -6, int hi = -1)
{
    std::vector<float> w((size_t)cout * cin * 9);
    for (size_t i = 0; i < w.size(); i++) w[i] = rnd_float(lo, hi);
    return w;
}
static float W(const std::vector<float> &w, int cin, int o, int c, int tap) { return w[((size_t)o * cin + c) * 9 + tap]; }

// an image under test: poisoned before the packer runs, every documented address visited once, everything else must be +0 / -0
template <typename T> struct Image {
    std::vector<T> v;
    std::vector<char> seen;
    explicit Image(size_t n) : v(n), seen(n, 0) { std::memset(v.data(), 0xFF, n * sizeof(T)); }
    bool at(size_t i, T *out)
    {
        if (i >= v.size() || seen[i]) return false;   // outside the image, or two weights at one address
        seen[i] = 1;
        *out = v[i];
        return true;
    }
    long first_nonzero_padding() const
    {
        for (size_t i = 0; i < v.size(); i++)
            if (!seen[i] && !(v[i] == 0)) return (long)i;
        return -1;
    }
};

static const int MID[3] = {32, 64, 128};

// ---- the fp32 images of w2xc_kernels.hip (layouts: the comment on w2xc_pack_weights) ----
static void test_pack_weights_addresses()
{
    struct Shape { W2xcKernelKind kind; int cin, cout; };
    std::vector<Shape> shapes;
    for (int a : MID)
        for (int b : MID) shapes.push_back({W2XC_K_MFMA, a, b});
    for (int a : {1, 3})
        for (int b : MID) { shapes.push_back({W2XC_K_FIRST, a, b}); shapes.push_back({W2XC_K_FIRST_SPLIT, a, b}); }
    for (int a : MID)
        for (int b : {1, 3}) shapes.push_back({W2XC_K_LAST, a, b});
    for (int a : {1, 3, 5, 32})
        for (int b : {1, 3, 7, 8, 9, 32}) shapes.push_back({W2XC_K_DIRECT, a, b});
    for (const Shape &s : shapes) {
        const int cin = s.cin, cout = s.cout;
        const std::vector<float> w = weights(cout, cin);
        Image<float> img(w2xc_packed_weight_floats(s.kind, cin, cout));
        w2xc_pack_weights(s.kind, cin, cout, w.data(), img.v.data());
        for (int o = 0; o < cout; o++)
            for (int c = 0; c < cin; c++)
                for (int tap = 0; tap < 9; tap++) {
                    size_t i;
                    if (s.kind == W2XC_K_MFMA) {          // [tap][c / 8][nb][lane = 32 (c % 8) / 4 + o % 32][c % 4]
                        i = ((((size_t)tap * (cin / 8) + c / 8) * (cout / 32) + o / 32) * 64 + 32 * ((c % 8) / 4) + o % 32) * 4 + c % 4;
                    } else if (s.kind == W2XC_K_LAST) {   // [c / 16][c % 4][n / 16][lane = 16 (c % 16) / 4 + n % 16], n = tap * cout + o
                        const int n = tap * cout + o;
                        i = (((size_t)(c / 16) * 4 + c % 4) * ((9 * cout + 15) / 16) + n / 16) * 64 + 16 * ((c % 16) / 4) + n % 16;
                    } else if (s.kind == W2XC_K_DIRECT) {  // [c][tap][o], rows padded to 8
                        i = ((size_t)c * 9 + tap) * ((cout + 7) / 8 * 8) + o;
                    } else {                               // first layer: [nb][k / 2][lane = 32 (k % 2) + o % 32], k = 9 c + tap
                        const int k = 9 * c + tap;
                        i = ((size_t)(o / 32) * ((9 * cin + 1) / 2) + k / 2) * 64 + 32 * (k % 2) + o % 32;
                    }
                    float got;
                    CHECK(img.at(i, &got) && got == W(w, cin, o, c, tap), "kind %d %d->%d: W[%d][%d][%d] not at %zu", (int)s.kind, cin, cout, o, c, tap, i);
                }
        CHECK(img.first_nonzero_padding() < 0, "kind %d %d->%d: padding slot %ld is not 0", (int)s.kind, cin, cout, img.first_nonzero_padding());
    }
}

// ---- Winograd images: U = G g G^T in long double from G's definition (rows = the filter evaluated at a point / the product of the point's
//      distances to the others; last row = the leading coefficient), against the image value rounded once from double: within one fp32 ulp ----
template <int N>
static void transformed(const long double (&G)[N][3], const float *g, long double (&U)[N][N])
{
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            long double u = 0;
            for (int r = 0; r < 3; r++)
                for (int s = 0; s < 3; s++) u += G[i][r] * (long double)g[3 * r + s] * G[j][s];
            U[i][j] = u;
        }
}
template <int NP>
static void cook_toom_G(const long double (&pts)[NP], long double (&G)[NP + 1][3])
{
    for (int i = 0; i < NP; i++) {
        long double den = 1;
        for (int k = 0; k < NP; k++)
            if (k != i) den *= pts[i] - pts[k];
        G[i][0] = 1 / den; G[i][1] = pts[i] / den; G[i][2] = pts[i] * pts[i] / den;
    }
    G[NP][0] = 0; G[NP][1] = 0; G[NP][2] = 1;
}
static bool close_ulp(float got, long double want, long double mag) { return std::fabs((long double)got - want) <= std::ldexp(mag, -23); }
template <int N>
static long double mag_of(const long double (&U)[N][N], int i, int j) { return std::fabs(U[i][j]) > 0 ? std::fabs(U[i][j]) : 1e-30L; }

static void test_wino_addresses()
{
    // F(2x2,3x3), points 0, 1, -1 (G scaled as the kernel's B^T and A^T expect: rows 1/2 (1, +-1, 1))
    const long double G[4][3] = {{1, 0, 0}, {0.5L, 0.5L, 0.5L}, {0.5L, -0.5L, 0.5L}, {0, 0, 1}};
    for (int cin : MID)
        for (int cout : MID) {
            CHECK(w2xc_wino_supported(cin, cout), "%d->%d", cin, cout);
            const std::vector<float> w = weights(cout, cin);
            Image<float> img(w2xc_wino_packed_floats(cin, cout));
            w2xc_wino_pack(cin, cout, w.data(), img.v.data());
            for (int o = 0; o < cout; o++)
                for (int c = 0; c < cin; c++) {
                    long double U[4][4];
                    transformed(G, &w[((size_t)o * cin + c) * 9], U);
                    for (int xi = 0; xi < 16; xi++) {   // [o / 32][c / 16][(c % 8) / 2][c % 2][xi / 4][lane = 32 (c % 16) / 8 + o % 32][xi % 4]
                        const size_t i = ((((((size_t)(o / 32) * (cin / 16) + c / 16) * 4 + (c % 8) / 2) * 2 + c % 2) * 4 + xi / 4) * 64 + 32 * ((c % 16) / 8) + o % 32) * 4 + xi % 4;
                        float got;
                        CHECK(img.at(i, &got) && close_ulp(got, U[xi / 4][xi % 4], mag_of(U, xi / 4, xi % 4)), "%d->%d: U_%d[%d][%d] not at %zu", cin, cout, xi, o, c, i);
                    }
                }
            CHECK(img.first_nonzero_padding() < 0, "%d->%d: slot %ld never addressed and not 0", cin, cout, img.first_nonzero_padding());
        }
}

static void wino4_G(long double (&G)[6][3])
{
    const long double pts[5] = {0, 0.75L, -0.75L, 1.5L, -1.5L};
    cook_toom_G(pts, G);
}
// position (i, j) in conv3x3_wino4's fragment order: the column halves j < 3 / j >= 3 as the xi ranges [0, 18) / [18, 36)
static int wino4_xi(int i, int j) { return (j < 3 ? 0 : 18) + 3 * i + j % 3; }
static size_t wino4_index(int cin, int o, int c, int xi)   // [o / 64][c / 4][xi / 4][(o % 64) / 16][lane = 16 (c % 4) + o % 16][xi % 4]
{
    return (((((size_t)(o / 64) * (cin / 4) + c / 4) * 9 + xi / 4) * 4 + (o % 64) / 16) * 64 + 16 * (c % 4) + o % 16) * 4 + xi % 4;
}
static size_t first2_index(int o, int c, int xi)           // [xi / 9][xi % 9][o / 16][c / 4][lane = 16 (c % 4) + o % 16], xi = 6 i + j
{
    return ((((size_t)(xi / 9) * 9 + xi % 9) * 2 + o / 16) * 8 + c / 4) * 64 + 16 * (c % 4) + o % 16;
}

static void test_wino4_addresses()
{
    long double G[6][3];
    wino4_G(G);
    for (int cin : MID)
        for (int cout : {64, 128}) {
            CHECK(w2xc_wino4_supported(cin, cout), "%d->%d", cin, cout);
            const std::vector<float> w = weights(cout, cin);
            Image<float> img((size_t)36 * cin * cout);
            w2xc_wino4_pack(cin, cout, w.data(), img.v.data());
            for (int o = 0; o < cout; o++)
                for (int c = 0; c < cin; c++) {
                    long double U[6][6];
                    transformed(G, &w[((size_t)o * cin + c) * 9], U);
                    for (int i = 0; i < 6; i++)
                        for (int j = 0; j < 6; j++) {
                            float got;
                            const size_t at = wino4_index(cin, o, c, wino4_xi(i, j));
                            CHECK(img.at(at, &got) && close_ulp(got, U[i][j], mag_of(U, i, j)), "%d->%d: U(%d,%d)[%d][%d] not at %zu", cin, cout, i, j, o, c, at);
                        }
                }
            CHECK(img.first_nonzero_padding() < 0, "%d->%d: slot %ld never addressed and not 0", cin, cout, img.first_nonzero_padding());
        }
}

// conv3x3_first2_wino4's image, and: both F(4x4,3x3) packers hold the same U bit for bit.  (w2xc_wino4_pack works in blocks of 64 output planes: the
// 32 -> 32 layer's filters are planes 0..31 of a 32 -> 64 image -- U of a (plane, channel) pair depends on that pair's filter alone.)
static void test_first2_wino4_addresses_and_agreement()
{
    long double G[6][3];
    wino4_G(G);
    CHECK(w2xc_first2_wino4_supported(1, 32, 32) && !w2xc_first2_wino4_supported(3, 32, 32) && !w2xc_first2_wino4_supported(1, 32, 64), "predicate");
    std::vector<float> w = weights(64, 32);
    Image<float> a((size_t)36 * 32 * 32), b((size_t)36 * 32 * 64);
    w2xc_first2_wino4_pack(w.data(), a.v.data());
    w2xc_wino4_pack(32, 64, w.data(), b.v.data());
    for (int o = 0; o < 32; o++)
        for (int c = 0; c < 32; c++) {
            long double U[6][6];
            transformed(G, &w[((size_t)o * 32 + c) * 9], U);
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < 6; j++) {
                    float ga = 0, gb = 0;
                    CHECK(a.at(first2_index(o, c, 6 * i + j), &ga) && close_ulp(ga, U[i][j], mag_of(U, i, j)), "U(%d,%d)[%d][%d] not at %zu", i, j, o, c, first2_index(o, c, 6 * i + j));
                    CHECK(b.at(wino4_index(32, o, c, wino4_xi(i, j)), &gb) && std::memcmp(&ga, &gb, 4) == 0, "U(%d,%d)[%d][%d]: the two packers disagree (%a, %a)", i, j, o, c, ga, gb);
                }
        }
    CHECK(a.first_nonzero_padding() < 0, "slot %ld never addressed and not 0", a.first_nonzero_padding());
}

static void test_wino4_pack_last_addresses()
{
    for (int cin : {32, 64, 128}) {
        const std::vector<float> w = weights(1, cin);
        Image<float> img(w2xc_wino4_pack_last_floats(cin));
        w2xc_wino4_pack_last(cin, w.data(), img.v.data());
        for (int c = 0; c < cin; c++)
            for (int tap = 0; tap < 9; tap++) {   // [c / 16][c % 4][lane = 16 (c % 16) / 4 + tap]
                const size_t i = ((size_t)(c / 16) * 4 + c % 4) * 64 + 16 * ((c % 16) / 4) + tap;
                float got;
                CHECK(img.at(i, &got) && got == W(w, cin, 0, c, tap), "cin %d: W[%d][%d] not at %zu", cin, c, tap, i);
            }
        CHECK(img.first_nonzero_padding() < 0, "cin %d: padding slot %ld (taps 9..15) is not 0", cin, img.first_nonzero_padding());
    }
}

// ---- split images: 16-bit terms ----
static double bf16_val(uint16_t h)
{
    const uint32_t u = (uint32_t)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static double fp16_val(uint16_t h)
{
    const int e = (h >> 10) & 31, m = h & 0x3FF;
    const double a = e == 31 ? INFINITY : e ? std::ldexp((double)(m | 0x400), e - 25) : std::ldexp((double)m, -24);
    return (h & 0x8000) ? -a : a;
}
static bool is_pow2(float s) { int e; return s > 0 && std::frexp(s, &e) == 0.5f; }

// one weight and its `terms` terms against what the formats promise.  Returns NULL or the name of the broken promise.
//   bf16 (8-bit significand, fp32's exponent range), round to nearest: every rounding is off by at most half an ulp = 2^-8 of the rounded value's
//   binade, so  one term |w - t0| <= 2^-8 |w|;  two terms  <= 2^-16 |w|;  three terms: the residuals are multiples of w's last bit below 2^-8, 2^-16 of
//   w's binade, i.e. 16 and then 8 significant bits: the third term takes what is left, t0 + t1 + t2 == w;  and each term is at most 2^-8 of the one before.
//   fp16 (11-bit significand, subnormal spacing 2^-24), two terms of v = S w: |v - (h0 + h1)| <= max(2^-22 |v|, 2^-25).
static const char *terms_hold(double v, const uint16_t *t, int terms, int fmt)
{
    double x[3] = {0, 0, 0};
    for (int k = 0; k < terms; k++) x[k] = fmt ? fp16_val(t[k]) : bf16_val(t[k]);
    const double sum = x[0] + x[1] + x[2], err = std::fabs(v - sum), av = std::fabs(v);   // (exact in double: the terms span < 53 bits)
    if (fmt == 1) return err <= std::fmax(std::ldexp(av, -22), std::ldexp(1.0, -25)) ? nullptr : "fp16 x 2: |S w - (h0 + h1)| <= max(2^-22 |S w|, 2^-25)";
    for (int k = 1; k < terms; k++)
        if (std::fabs(x[k]) > std::ldexp(std::fabs(x[k - 1]), -8)) return "a term is at most 2^-8 of the one before";
    if (terms == 3) return err == 0 ? nullptr : "bf16 x 3: t0 + t1 + t2 == w";
    return err <= std::ldexp(av, -8 * terms) ? nullptr : "bf16: |w - sum| <= 2^(-8 terms) |w|";
}

static void check_split(int cin, int cout, int terms, int fmt, const std::vector<float> &w, bool zeros)
{
    Image<uint16_t> img(w2xc_split_packed_bytes(cin, cout, terms) / 2);
    const float S = w2xc_split_pack(cin, cout, terms, fmt, w.data(), img.v.data());
    float mx = 0;
    for (float f : w) mx = std::fmax(mx, std::fabs(f));
    if (fmt == 0 || zeros) CHECK(S == 1.0f, "%d->%d terms %d fmt %d: scale %a", cin, cout, terms, fmt, S);
    else CHECK(is_pow2(S) && S * mx >= 16384.0f && S * mx < 32768.0f, "%d->%d fmt 1: scale %a puts max|w| = %a at %a", cin, cout, S, mx, S * mx);
    const int kg = w2xc_split_kg(terms, cin), nsl = cin / (16 * kg), nbt = cout / 32;
    CHECK(kg == (terms == 1 ? (cin >= 64 ? 4 : 2) : 1), "kg");
    for (int o = 0; o < cout; o++)
        for (int c = 0; c < cin; c++)
            for (int tap = 0; tap < 9; tap++) {
                uint16_t t[3] = {0, 0, 0};
                const int sl = c / (16 * kg), g = (c % (16 * kg)) / 16, lane = 32 * ((c % 16) / 8) + o % 32, e = c % 8;
                for (int k = 0; k < terms; k++) {   // [tap][slice][term][g][nb][lane][e]
                    const size_t i = ((((((size_t)tap * nsl + sl) * terms + k) * kg + g) * nbt + o / 32) * 64 + lane) * 8 + e;
                    CHECK(img.at(i, &t[k]), "%d->%d terms %d: term %d of W[%d][%d][%d]: address %zu", cin, cout, terms, k, o, c, tap, i);
                }
                const char *broken = terms_hold((double)S * W(w, cin, o, c, tap), t, terms, fmt);
                CHECK(!broken, "%d->%d terms %d fmt %d: W[%d][%d][%d] = %a, terms %04x %04x %04x: %s", cin, cout, terms, fmt, o, c, tap, W(w, cin, o, c, tap), t[0], t[1], t[2], broken);
            }
    CHECK(img.first_nonzero_padding() < 0, "%d->%d terms %d: slot %ld never addressed and not 0", cin, cout, terms, img.first_nonzero_padding());
}

static void check_split_last(int cin, int terms, int fmt, const std::vector<float> &w, bool zeros)
{
    Image<uint16_t> img(w2xc_split_pack_last_bytes(cin, terms) / 2);
    const float S = w2xc_split_pack_last(cin, terms, fmt, w.data(), img.v.data());
    float mx = 0;
    for (float f : w) mx = std::fmax(mx, std::fabs(f));
    if (fmt == 0 || zeros) CHECK(S == 1.0f, "cin %d terms %d fmt %d: scale %a", cin, terms, fmt, S);
    else CHECK(is_pow2(S) && S * mx >= 16384.0f && S * mx < 32768.0f, "cin %d fmt 1: scale %a puts max|w| = %a at %a", cin, S, mx, S * mx);
    for (int c = 0; c < cin; c++)
        for (int tap = 0; tap < 9; tap++) {
            // [term][c / 32][h = (c % 32) / 16][lane = 32 kk + tap][e]: channel 16 h + 4 kk + (e < 4 ? e : 4 + e), the order of accumulator registers 8 h .. 8 h + 7
            const int r = c % 16, kk = (r / 4) % 2, e = r % 4 + 4 * (r / 8);
            uint16_t t[3] = {0, 0, 0};
            for (int k = 0; k < terms; k++) {
                const size_t i = ((((size_t)k * (cin / 32) + c / 32) * 2 + (c % 32) / 16) * 64 + 32 * kk + tap) * 8 + e;
                CHECK(img.at(i, &t[k]), "cin %d terms %d: term %d of W[%d][%d]: address %zu", cin, terms, k, c, tap, i);
            }
            const char *broken = terms_hold((double)S * W(w, cin, 0, c, tap), t, terms, fmt);
            CHECK(!broken, "cin %d terms %d fmt %d: W[%d][%d] = %a, terms %04x %04x %04x: %s", cin, terms, fmt, c, tap, W(w, cin, 0, c, tap), t[0], t[1], t[2], broken);
        }
    CHECK(img.first_nonzero_padding() < 0, "cin %d terms %d: padding slot %ld (taps 9..31) is not 0", cin, terms, img.first_nonzero_padding());
}

static void test_split_images()
{
    const int modes[4][2] = {{1, 0}, {2, 0}, {3, 0}, {2, 1}};   // (terms, fmt)
    for (int cin : MID)
        for (int cout : MID)
            for (const int (&m)[2] : modes) {
                // bf16: weights of "ordinary magnitude" 2^-100 .. 2^100 (far from fp32's own under- and overflow); fp16 scales to its range itself
                check_split(cin, cout, m[0], m[1], m[1] ? weights(cout, cin, -30, 3) : weights(cout, cin, -100, 100), false);
                if (g_failed) return;
            }
    for (int cin : MID)
        for (const int (&m)[2] : modes) {
            check_split_last(cin, m[0], m[1], m[1] ? weights(1, cin, -30, 3) : weights(1, cin, -100, 100), false);
            if (g_failed) return;
        }
    // fp16 scale: all zeros -> 1; a maximum that is an exact power of two must land on 2^14, the closed end of [2^14, 2^15)
    std::vector<float> z((size_t)64 * 32 * 9, 0.0f), p = weights(64, 32, -9, -4);
    p[777] = -0.125f;
    check_split(32, 64, 2, 1, z, true);
    check_split(32, 64, 2, 1, p, false);
    z.resize(64 * 9); p.resize(64 * 9);
    p[5] = 0.5f;
    check_split_last(64, 2, 1, z, true);
    check_split_last(64, 2, 1, p, false);
}

static void test_prog_counters()
{
    for (int w = 1; w <= 4100; w += (w < 600 ? 1 : 97))
        for (int h = 1; h <= 2200; h += (h < 100 ? 1 : 53))
            for (int py = 0; py < 4; py++) {
                int rows = -1, groups = -1;
                w2xc_wino4_prog_jobs(w, h, py, &rows, &groups);
                // the grid covers the region: rows of 16 starting py rows above it, groups of 8 tiles of 32 columns -- and not a whole row / group more
                CHECK(rows * 16 >= h + py && (rows - 1) * 16 < h + py && groups * 256 >= w && (groups - 1) * 256 < w, "w=%d h=%d py=%d: %d x %d jobs", w, h, py, rows, groups);
                CHECK(w2xc_wino4_prog_counters(w, h, py) == 2 * (size_t)rows * groups + 2, "w=%d h=%d py=%d: %zu counters for %d x %d jobs", w, h, py,
                      w2xc_wino4_prog_counters(w, h, py), rows, groups);
            }
}

int main()
{
    test_pack_weights_addresses();
    test_wino_addresses();
    test_wino4_addresses();
    test_first2_wino4_addresses_and_agreement();
    test_wino4_pack_last_addresses();
    test_split_images();
    test_prog_counters();
    std::printf(g_failed ? "%d properties FAILED\n" : "all packer properties hold\n", g_failed);
    return g_failed;
}
