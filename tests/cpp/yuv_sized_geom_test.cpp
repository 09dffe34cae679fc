// tests/cpp/yuv_sized_geom_test.cpp -- the integers and doubles of "Sized YUV frames" in w2xc_host_geom.hpp, on the CPU (no HIP, no library: the header
// alone, as host_geom_test.cpp takes it; tests/test_yuv_sized_api.py builds and runs it):
//   * the window of k_chroma_resize_u8 / _u16: for every tile of 32 (16) OUTPUT samples of an axis, every output's four taps lie inside the 35 (19) source
//     samples that start at chroma_resize_origin of the tile's first output -- over a sweep of luma sizes, ratios <= 1, both offsets;
//   * at r = 0.5 the positions are those of the 2x kernels (s = q - 1 for m = 2q - 1 and 2q, t = 0.25 / 0.75 or 0.375 / 0.875), at r = 1 they are (m, 0);
//   * W2XC_ITERATIONS_AUTO's rule, the float planes of a sized call, the launch grid.
#include "../../waifu2x-converter-cpp_amd/csrc/w2xc_host_geom.hpp"

#include <cstdio>

using namespace w2xc_eng;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                 \
    } while (0)

// one axis: n_out output chroma samples, tiles of `tile` outputs, a window of tile + 3 source samples
static long long check_axis(int luma_in, int luma_out, bool sub, bool cosited, int tile)
{
    const ChromaAxis a = chroma_axis(luma_in, luma_out, sub, cosited);
    const int n_out = sub ? (luma_out + 1) / 2 : luma_out;
    long long checked = 0;
    CHECK(a.r > 0.0 && a.r <= 1.0, "%d -> %d: r = %g", luma_in, luma_out, a.r);
    int last = -(1 << 30);
    for (int m0 = 0; m0 < n_out; m0 += tile) {
        const int g0 = chroma_resize_origin(m0, a.r, a.o);
        for (int m = m0; m < m0 + tile && m < n_out; m++) {
            const double pos = chroma_resize_pos(m, a.r, a.o);
            const int s = chroma_resize_floor(pos);
            const double t = pos - s;
            CHECK(t >= 0.0 && t < 1.0, "%d -> %d o=%g m=%d: t = %g", luma_in, luma_out, a.o, m, t);
            CHECK(s >= last, "%d -> %d o=%g m=%d: the floors go down (%d after %d)", luma_in, luma_out, a.o, m, s, last);
            CHECK(s - last <= 1 || m == 0, "%d -> %d o=%g m=%d: the floors skip a sample (%d after %d)", luma_in, luma_out, a.o, m, s, last);
            last = s;
            const int c0 = s - 1 - g0;   // the window column of tap 0
            CHECK(c0 >= 0 && c0 + 3 <= tile + 2, "%d -> %d o=%g tile at %d, m=%d: taps at window columns %d .. %d of %d", luma_in, luma_out, a.o, m0, m, c0, c0 + 3,
                  tile + 3);
            checked++;
        }
    }
    return checked;
}

int main()
{
    long long checked = 0;
    // luma sizes around tile edges, odd and even, small and video-sized; every output size from the input's to 4x (16x for the small ones)
    const int ins[] = {1, 2, 3, 5, 7, 31, 32, 33, 63, 64, 65, 127, 360, 480, 540, 719, 720, 1080, 1440};
    for (int in : ins)
        for (int sub = 0; sub < 2; sub++)
            for (int cos = 0; cos <= sub; cos++) {
                const int top = in <= 65 ? 16 * in : 4 * in, step = in <= 127 ? 1 : 7;
                for (int out = in; out <= top; out += step) {
                    checked += check_axis(in, out, sub, cos, 32);
                    checked += check_axis(in, out, sub, cos, 16);
                }
                checked += check_axis(in, top, sub, cos, 32);
            }
    // the ratios the issue names, and the largest sizes a call takes
    const int pairs[][2] = {{1280, 1920}, {720, 1080}, {960, 3840}, {540, 2160}, {720, 1920}, {480, 1080}, {1440, 3840}, {1 << 22, 1 << 22}, {(1 << 22) - 1, 1 << 22},
                            {1 << 18, 1 << 22}, {(1 << 18) + 1, 1 << 22}};
    for (const auto &p : pairs)
        for (int sub = 0; sub < 2; sub++)
            for (int cos = 0; cos <= sub; cos++) checked += check_axis(p[0], p[1], sub, cos, 32) + check_axis(p[0], p[1], sub, cos, 16);

    // r = 0.5 is the 2x kernels' geometry, r = 1 the identity's
    for (int cos = 0; cos < 2; cos++) {
        const ChromaAxis a = chroma_axis(100, 200, true, cos);
        CHECK(a.r == 0.5, "r = %g", a.r);
        for (int q = 0; q < 70; q++) {
            for (int odd = 0; odd < 2; odd++) {
                const int m = 2 * q - odd;
                if (m < 0) continue;
                const double pos = chroma_resize_pos(m, a.r, a.o);
                const int s = chroma_resize_floor(pos);
                const double want = cos ? (odd ? 0.375 : 0.875) : (odd ? 0.25 : 0.75);
                CHECK(s == q - 1 && pos - s == want, "r = 0.5 cos=%d m=%d: s = %d, t = %g", cos, m, s, pos - s);
            }
        }
        for (int q0 = 0; q0 < 128; q0 += 16) CHECK(chroma_resize_origin(2 * q0, a.r, a.o) == q0 - 2, "the 2x window's origin at quad %d", q0);
        const ChromaAxis one = chroma_axis(77, 77, true, cos);
        for (int m = 0; m < 77; m++) CHECK(chroma_resize_pos(m, one.r, one.o) == (double)m, "r = 1: pos(%d) = %g", m, chroma_resize_pos(m, one.r, one.o));
    }
    CHECK(chroma_axis(8, 8, false, true).o == 0.5, "a flag on an axis that is not subsampled does not move it");

    // W2XC_ITERATIONS_AUTO
    const int autos[][5] = {{1280, 720, 1920, 1080, 1}, {1920, 1080, 3840, 2160, 1}, {960, 540, 3840, 2160, 2}, {720, 480, 1920, 1080, 2}, {1440, 1080, 3840, 2160, 2},
                            {64, 64, 64, 64, 0}, {64, 64, 65, 64, 1}, {64, 64, 64, 129, 2}, {10, 10, 160, 160, 4}, {10, 10, 161, 10, 5}, {3, 5, 4, 9, 1}};
    for (const auto &c : autos) CHECK(sized_auto_iterations(c[0], c[1], c[2], c[3]) == c[4], "AUTO %dx%d -> %dx%d: %d", c[0], c[1], c[2], c[3], sized_auto_iterations(c[0], c[1], c[2], c[3]));

    // the float planes: a sized call at its last level takes what the base call takes; below it, one more plane (three on the RGB route) of the output's size
    for (int it = 0; it <= 4; it++) {
        const int w = 37, h = 21, W = w << it, H = h << it;
        size_t y = 2 * plane_floats(w, h), rgb = plane_floats(w, h);
        for (int i = 1; i <= it; i++) { y += 2 * plane_floats(w << i, h << i); rgb += plane_floats(w << i, h << i); }
        CHECK(yuv_aux_floats(w, h, it) == y && yuv_aux_floats(w, h, it, W, H) == y, "it=%d: the Y route's planes", it);
        CHECK(yuv_rgb_aux_floats(false, w, h, it) == 3 * rgb && yuv_rgb_aux_floats(true, w, h, it, W, H) == 3 * (rgb + plane_floats(w, h)), "it=%d: the RGB route's planes", it);
        if (it) {
            CHECK(yuv_aux_floats(w, h, it, W - 1, H) == y + plane_floats(W - 1, H), "it=%d: the shrunk luma plane", it);
            CHECK(yuv_rgb_aux_floats(false, w, h, it, W, H - 3) == 3 * (rgb + plane_floats(W, H - 3)), "it=%d: the shrunk RGB planes", it);
        }
    }

    // the grid: tiles of 32 x 16 outputs, per_tile turns each, capped
    const YuvTileGrid g = chroma_resize_tile_grid(960, 540, 16, 32, 16, 2048), one = chroma_resize_tile_grid(1, 1, 1, 32, 16, 2048),
                      edge = chroma_resize_tile_grid(33, 17, 3, 32, 16, 2048);
    CHECK(g.tiles_x == 30 && g.tiles == 30 * 34 && g.turns == 30 * 34 * 16 && g.grid == 2048, "the grid of 1080p chroma");
    CHECK(one.tiles == 1 && one.turns == 1 && one.grid == 1, "the grid of one sample");
    CHECK(edge.tiles_x == 2 && edge.tiles == 4 && edge.turns == 12 && edge.grid == 12, "the grid one past a tile edge");

    if (failures) { std::printf("%d sized-frame geometry checks FAILED\n", failures); return 1; }
    std::printf("all sized-frame geometry properties hold (%lld output positions)\n", checked);
    return 0;
}
