// upconv_alpha_pack_test.cpp -- the weight image of the alpha head (w2xc_upconv_pack_alpha, waifu2x-converter-cpp_amd/csrc/w2xc_pack.cpp) checked on the CPU:
// built with g++ from that file alone, like upconv_pack_test.cpp.  upconv4x4_head<C, 1, true> computes channel 1 of a three-plane head by itself; its bytes
// equal channel 1 of the full head because its B operand is, column for column, what the full head's B operand holds for that channel:
//   * column 4 r + s of the image packed from Wt[:, 1] equals column (4 r + s) * 3 + 1 of the three-output image, for every MFMA step and lane row;
//   * the image is w2xc_upconv_pack(C, 1, .) on the slice Wt[:, 1], float for float, and has 16 C floats.
// Prints the first failing input of each property; exit status = number of failed properties.
#include "../../waifu2x-converter-cpp_amd/csrc/w2xc_pack.hpp"

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

static void alpha_image(int cin)
{
    const int nout = 3;
    const size_t nw = (size_t)cin * nout * 16;
    std::vector<float> w(nw);
    for (size_t i = 0; i < nw; i++) w[i] = (float)(i + 1);   // distinct, exact in fp32
    std::vector<float> full(w2xc_upconv_packed_floats(cin, nout), -1.0f), one(w2xc_upconv_packed_floats(cin, 1), -1.0f);
    CHECK(one.size() == (size_t)16 * cin, "%d: %zu floats", cin, one.size());
    w2xc_upconv_pack(cin, nout, w.data(), full.data());
    w2xc_upconv_pack_alpha(cin, w.data(), one.data());
    // the image is [step = (g, j)][block nb][lane]: lane & 15 = the column inside the block, lane >> 4 = the k row of the step
    for (int step = 0; step < cin / 4; step++)
        for (int k = 0; k < 4; k++)
            for (int tap = 0; tap < 16; tap++) {
                const int n3 = tap * 3 + 1;   // the column of (tap, channel 1) in the three-output image
                const float a = one[((size_t)step * 1 + 0) * 64 + 16 * k + tap];
                const float b = full[((size_t)step * 3 + n3 / 16) * 64 + 16 * k + n3 % 16];
                CHECK(a == b, "%d: step %d row %d column %d holds %g, column %d of the full image %g", cin, step, k, tap, a, n3, b);
            }
    // ... and it is the one-output packer on the slice Wt[:, 1]
    std::vector<float> w1((size_t)cin * 16), ref(one.size(), -2.0f);
    for (int c = 0; c < cin; c++) std::memcpy(&w1[(size_t)c * 16], &w[((size_t)c * 3 + 1) * 16], 16 * sizeof(float));
    w2xc_upconv_pack(cin, 1, w1.data(), ref.data());
    for (size_t i = 0; i < one.size(); i++) CHECK(one[i] == ref[i], "%d: slot %zu holds %g, the packer on the slice %g", cin, i, one[i], ref[i]);
}

int main()
{
    for (int cin : {32, 64, 128, 256}) alpha_image(cin);
    if (g_failed) return g_failed;
    if (std::strcmp(w2xc_kernel_name(W2XC_K_UPCONV_A_U8, 256, 3), "upconv4x4_head_alpha_u8")) { std::printf("FAIL name\n"); return 1; }
    std::printf("all alpha head packer properties hold\n");
    return 0;
}
