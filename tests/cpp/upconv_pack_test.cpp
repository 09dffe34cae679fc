// upconv_pack_test.cpp -- the packers of upconv head models (waifu2x-converter-cpp_amd/csrc/w2xc_pack.cpp) checked as properties on the CPU: built with g++
// from that file alone (no HIP, no library), like pack_test.cpp.  What is asserted is what upconv4x4_head (w2xc_upconv.hip) needs:
//   * every weight Wt[c][o][r][s] appears in the head image exactly once, at the lane its (c, tap, o) says -- the A / B fragment addressing of
//     v_mfma_f32_16x16x4_f32 written out independently here -- and the image has no other slot;
//   * the zero-padded images of a head model's narrow layers (16 -> 32 planes) hold the model's weights where they were and exact zeros in every added plane;
//   * the grid rule and the kernel names.
// Prints the first failing input of each property; exit status = number of failed properties.
#include "../../waifu2x-converter-cpp_amd/csrc/w2xc_pack.hpp"

#include <cmath>
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

// distinct non-zero values: weight number i is i + 1 (exact in fp32 up to 2^24)
static std::vector<float> numbered(size_t n)
{
    std::vector<float> w(n);
    for (size_t i = 0; i < n; i++) w[i] = (float)(i + 1);
    return w;
}

static void head_image(int cin, int nout)
{
    const size_t nw = (size_t)cin * nout * 16;
    CHECK(w2xc_upconv_supported(cin, nout), "%d -> %d", cin, nout);
    CHECK(w2xc_upconv_packed_floats(cin, nout) == nw, "%d -> %d: %zu floats for %zu weights", cin, nout, w2xc_upconv_packed_floats(cin, nout), nw);
    const std::vector<float> w = numbered(nw);
    std::vector<float> img(nw, -1.0f);
    w2xc_upconv_pack(cin, nout, w.data(), img.data());
    std::vector<int> hits(nw, 0);
    for (int c = 0; c < cin; c++)
        for (int tap = 0; tap < 16; tap++)
            for (int o = 0; o < nout; o++) {
                // MFMA step (g, j) of the kernel contracts the planes 16 g + 4 k + j, k = lane >> 4; column n = tap * nout + o sits in block n / 16 at lane & 15 = n % 16
                const int g = c / 16, k = (c % 16) / 4, j = c % 4, n = tap * nout + o;
                const size_t at = (((size_t)g * 4 + j) * nout + n / 16) * 64 + 16 * k + n % 16;
                CHECK(at < nw, "%d -> %d: (c %d, tap %d, o %d) outside the image", cin, nout, c, tap, o);
                CHECK(img[at] == w[((size_t)c * nout + o) * 16 + tap], "%d -> %d: (c %d, tap %d, o %d) at %zu holds %g", cin, nout, c, tap, o, at, img[at]);
                hits[at]++;
            }
    for (size_t i = 0; i < nw; i++) CHECK(hits[i] == 1, "%d -> %d: slot %zu holds %d weights", cin, nout, i, hits[i]);
}

static void padded_layer()
{
    const int cin = 3, cout = 16, cout_p = 32;
    const std::vector<float> w = numbered((size_t)cout * cin * 9);
    std::vector<float> p((size_t)cout_p * cin * 9, -1.0f);
    w2xc_pad_layer(cin, cout, cin, cout_p, w.data(), p.data());   // 3 -> 16 as 3 -> 32: added OUTPUT planes
    for (int o = 0; o < cout_p; o++)
        for (int i = 0; i < cin; i++)
            for (int t = 0; t < 9; t++) {
                const float v = p[((size_t)o * cin + i) * 9 + t];
                if (o < cout) CHECK(v == w[((size_t)o * cin + i) * 9 + t], "3 -> 32: W[%d][%d][%d] = %g", o, i, t, v);
                else CHECK(v == 0.0f && !std::signbit(v), "3 -> 32: added plane %d holds %g", o, v);
            }
    const int cin2 = 16, cin2_p = 32, cout2 = 32;
    const std::vector<float> w2 = numbered((size_t)cout2 * cin2 * 9);
    std::vector<float> p2((size_t)cout2 * cin2_p * 9, -1.0f);
    w2xc_pad_layer(cin2, cout2, cin2_p, cout2, w2.data(), p2.data());   // 16 -> 32 as 32 -> 32: added INPUT planes
    for (int o = 0; o < cout2; o++)
        for (int i = 0; i < cin2_p; i++)
            for (int t = 0; t < 9; t++) {
                const float v = p2[((size_t)o * cin2_p + i) * 9 + t];
                if (i < cin2) CHECK(v == w2[((size_t)o * cin2 + i) * 9 + t], "32 -> 32: W[%d][%d][%d] = %g", o, i, t, v);
                else CHECK(v == 0.0f && !std::signbit(v), "32 -> 32: added input plane %d holds %g", i, v);
            }
    // ... and through the MFMA image of the padded layer: the zeros are zeros there too (every slot is a weight of the padded layer)
    std::vector<float> pk(w2xc_packed_weight_floats(W2XC_K_MFMA, cin2_p, cout2));
    w2xc_pack_weights(W2XC_K_MFMA, cin2_p, cout2, p2.data(), pk.data());
    size_t zeros = 0;
    for (float v : pk) zeros += v == 0.0f;
    CHECK(zeros == (size_t)cout2 * (cin2_p - cin2) * 9, "32 -> 32 image: %zu zeros", zeros);
    // a head behind a 16-plane layer: zero input planes behind the model's
    const int hc = 16, hc_p = 32, nout = 3;
    const std::vector<float> hw = numbered((size_t)hc * nout * 16);
    std::vector<float> hp((size_t)hc_p * nout * 16, -1.0f);
    w2xc_pad_head(hc, nout, hc_p, hw.data(), hp.data());
    for (size_t i = 0; i < hp.size(); i++) CHECK(hp[i] == (i < hw.size() ? hw[i] : 0.0f), "head 16 -> 32: slot %zu holds %g", i, hp[i]);
}

static void grid_and_names()
{
    for (int t : {1, 7, 511, 512}) CHECK(w2xc_upconv_grid(t) == t, "%d tiles: %d workgroups", t, w2xc_upconv_grid(t));
    for (int t : {513, 4096, 1 << 30}) CHECK(w2xc_upconv_grid(t) == 512, "%d tiles: %d workgroups", t, w2xc_upconv_grid(t));
    CHECK(!std::strcmp(w2xc_kernel_name(W2XC_K_UPCONV, 256, 3), "upconv4x4_head"), "name");
    CHECK(!std::strcmp(w2xc_kernel_name(W2XC_K_UPCONV_U8, 256, 3), "upconv4x4_head_u8"), "name");
    CHECK(!w2xc_upconv_supported(16, 3) && !w2xc_upconv_supported(48, 3) && !w2xc_upconv_supported(64, 2) && !w2xc_upconv_supported(512, 3), "shapes");
    // a plane count alone never selects the head, and the selection by shape is what it was
    CHECK(w2xc_pick_kernel(256, 3) == W2XC_K_DIRECT && w2xc_pick_kernel(128, 256) == W2XC_K_DIRECT && w2xc_pick_kernel(3, 16) == W2XC_K_DIRECT, "pick");
    CHECK(w2xc_pick_kernel(128, 3) == W2XC_K_LAST && w2xc_pick_kernel(32, 32) == W2XC_K_MFMA && w2xc_pick_kernel(3, 32) == W2XC_K_FIRST, "pick");
}

int main()
{
    for (int cin : {32, 64, 128, 256})
        for (int nout : {1, 3}) head_image(cin, nout);
    padded_layer();
    grid_and_names();
    if (!g_failed) std::printf("all upconv packer properties hold\n");
    return g_failed;
}
