// cuts_test.cpp -- the row cuts of the chunked launch strategies (waifu2x-converter-cpp_amd/csrc/w2xc_cuts.hpp) checked as properties on the CPU.
// Nothing here is taken from the code under test but the cuts themselves: the conditions are what the kernels behind the cuts need --
//   * the producer launches of a tail tile the producer's rows: nothing computed twice, nothing left out;
//   * the last layer's pieces tile the band's output rows in order, and none runs ahead of the producer rows it reads;
//   * a first-layer chunk waits for every view row a block it touches reads.
// Prints the first failing input of each property; exit status = number of failed properties.
#include "../../waifu2x-converter-cpp_amd/csrc/w2xc_cuts.hpp"

#include <cstdio>
#include <utility>
#include <vector>

using namespace w2xc_eng;
typedef std::vector<std::pair<int, int> > Spans;

static int g_failed = 0;
#define CHECK(cond, ...)                                               \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d: %s -- ", __func__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                  \
            std::printf("\n");                                         \
            g_failed++;                                                \
            return;                                                    \
        }                                                              \
    } while (0)

// do the spans tile [0, end) in order, each non-empty?
static bool tiles(const Spans &s, int end)
{
    int at = 0;
    for (size_t i = 0; i < s.size(); i++) {
        if (s[i].first != at || s[i].second <= at) return false;
        at = s[i].second;
    }
    return at == end;
}

// heights around every threshold of the cuts (128, 192, 256, the 32 / 48 / 64-row merge rules, 16-row tiles), the minimum sizes, the 2160-row frame
static std::vector<int> heights(int lo)
{
    std::vector<int> h;
    for (int r = lo; r <= 700; r++) h.push_back(r);
    const int mid[] = {720, 1023, 1024, 1025, 1080, 1081, 1440, 2047, 2048, 2049, 2159, 2160, 2161, 2162, 2176, 4320};
    for (size_t i = 0; i < sizeof mid / sizeof *mid; i++) h.push_back(mid[i]);
    return h;
}

// tail16: R >= 128 (the strategy's own condition).  The producer cuts lie TWO rows past a multiple of 16 -- the gather of rows [r0, r1) reads G rows up to
// r1 + 2, and it is the gather's cuts r1 that sit on 16-row tiles -- so "all but the last are multiples of 16" holds for the cuts less those two rows.
static void test_tail16()
{
    const std::vector<int> hs = heights(128);
    for (size_t i = 0; i < hs.size(); i++) {
        const int R = hs[i];
        Spans prod, out;
        int issued = 0, ahead = -1;
        cut_tail16(
            R, [&](int g0, int g1) { prod.push_back(std::make_pair(g0, g1)); issued = g1; return 0; },
            [&](int a, int b) { out.push_back(std::make_pair(a, b)); if (b + 2 > issued && ahead < 0) ahead = a; return 0; });
        CHECK(tiles(prod, R + 2), "R=%d: producer chunks do not tile [0, R + 2)", R);
        for (size_t j = 0; j + 1 < prod.size(); j++) CHECK((prod[j].second - 2) % 16 == 0, "R=%d: producer cut %d is not 2 past a 16-row tile", R, prod[j].second);
        CHECK(tiles(out, R), "R=%d: gather pieces do not tile [0, R)", R);
        CHECK(ahead < 0, "R=%d: the piece at row %d reads G rows no producer chunk has issued", R, ahead);
    }
}

// tail32: R >= 256; RL >= R + 2 + off_l (the producer's region holds every row the last layer reads), off_l 0 .. 6 (RowPlan::region)
static void test_tail32()
{
    const std::vector<int> hs = heights(256);
    const int widths[] = {4, 31, 32, 33, 255, 256, 1920, 1922, 3840, 3842};
    for (size_t i = 0; i < hs.size(); i++)
        for (int off_l = 0; off_l <= 6; off_l++)
            for (int extra = 0; extra <= 7; extra++)
                for (size_t wi = 0; wi < sizeof widths / sizeof *widths; wi++)
                    for (int blocks = 1; blocks <= 2; blocks++) {
                        const int R = hs[i], RL = R + 2 + off_l + extra, ipr = ((widths[wi] + 31) / 32) * blocks;
                        Spans prod, out;
                        int issued = 0, ahead = -1;
                        cut_tail32(
                            RL, R, off_l, ipr, [&](int p0, int p1) { prod.push_back(std::make_pair(p0, p1)); issued = p1; return 0; },
                            [&](int a, int b) { out.push_back(std::make_pair(a, b)); if (issued != RL && b + 2 + off_l > issued && ahead < 0) ahead = a; return 0; });
                        CHECK(tiles(prod, RL), "RL=%d R=%d off_l=%d items/row=%d: producer chunks do not tile [0, RL)", RL, R, off_l, ipr);
                        for (size_t j = 0; j + 1 < prod.size(); j++)
                            CHECK(prod[j].second % 16 == 0, "RL=%d R=%d off_l=%d items/row=%d: producer cut %d is not on a 16-row tile", RL, R, off_l, ipr, prod[j].second);
                        CHECK(tiles(out, R), "RL=%d R=%d off_l=%d items/row=%d: output pieces do not tile [0, R)", RL, R, off_l, ipr);
                        CHECK(ahead < 0, "RL=%d R=%d off_l=%d items/row=%d: the piece at row %d reads producer rows not yet issued", RL, R, off_l, ipr, ahead);
                    }
}

// the 2160x3840 frame, two 64-plane blocks: layer 6's region is rows [-1, 2161) = 2162 rows, 240 items per tile row: 64 + 48 + 24 tile rows
static void test_tail32_frame()
{
    Spans prod;
    cut_tail32(2162, 2160, 0, 240, [&](int p0, int p1) { prod.push_back(std::make_pair(p0, p1)); return 0; }, [](int, int) { return 0; });
    CHECK(prod.size() == 3, "%d producer chunks", (int)prod.size());
    const int want[3] = {64, 48, 24};
    for (int j = 0; j < 3; j++) {
        const int tile_rows = (prod[j].second - prod[j].first + 15) / 16;
        CHECK(tile_rows == want[j], "chunk %d: %d tile rows, expected %d", j, tile_rows, want[j]);
    }
}

// the last layer's taper: the host pipeline hands out multiples of 8 rows, min <= max; the strategy runs for out_h > max(min, 8)
static void test_taper()
{
    const std::vector<int> hs = heights(9);
    const int maxs[] = {8, 16, 64, 128, 136, 256, 512, 4096}, mins[] = {0, 8, 16, 32, 64};
    for (size_t i = 0; i < hs.size(); i++)
        for (size_t a = 0; a < sizeof maxs / sizeof *maxs; a++)
            for (size_t b = 0; b < sizeof mins / sizeof *mins; b++) {
                const int H = hs[i], mx = maxs[a], mn = mins[b];
                if (mn > mx || H <= std::max(mn, 8)) continue;
                Spans out;
                cut_taper(H, mx, mn, [&](int c0, int rows) { out.push_back(std::make_pair(c0, c0 + rows)); return 0; });
                CHECK(tiles(out, H), "out_h=%d max=%d min=%d: chunks do not tile [0, out_h)", H, mx, mn);
                for (size_t j = 0; j + 1 < out.size(); j++) {
                    const int rows = out[j].second - out[j].first;
                    CHECK(rows % 8 == 0 && rows <= mx, "out_h=%d max=%d min=%d: chunk of %d rows", H, mx, mn, rows);
                }
                CHECK(out.back().second - out.back().first < mx + std::max(mn, 8), "out_h=%d max=%d min=%d: last chunk of %d rows", H, mx, mn, out.back().second - out.back().first);
            }
}

// first-layer chunks: output rows [c0, c0 + rows) of a launch whose 4x4 blocks start at local rows = -wino_py mod 4.  Layer 1 alone: output row y reads
// rows y .. y + 2 of its input.  Layers 1 + 2 fused: a block that holds a row of the chunk is computed whole, and row y of layer 2 reads rows y .. y + 4.
static void test_first_chunk_last_row()
{
    const int steps[] = {8, 16, 24, 64, 512};
    for (int fused = 0; fused <= 1; fused++)
        for (int py = 0; py <= (fused ? 3 : 1); py++)
            for (int c0 = 0; c0 <= 96; c0 += 8)
                for (size_t si = 0; si < sizeof steps / sizeof *steps; si++)
                    for (int ragged = 0; ragged < 8; ragged++)          // (the last chunk of a launch ends where the region does)
                        for (int off_y = -30; off_y <= 12; off_y += 3)
                            for (int in_h = 1; in_h <= 700; in_h += 33) {
                                const int rows = steps[si] - ragged;
                                int need = c0 + rows - 1 + 2;
                                if (fused) {
                                    need = 0;
                                    for (int r = c0; r < c0 + rows; r++) {
                                        const int block = ((r + py) >> 2) * 4 - py;   // first local row of r's block
                                        need = std::max(need, block + 3 + 4);
                                    }
                                }
                                const int got = first_chunk_last_row(c0, rows, fused != 0, py, off_y, in_h);
                                CHECK(got >= 0 && got <= in_h - 1, "fused=%d py=%d c0=%d rows=%d off_y=%d in_h=%d: row %d outside the view", fused, py, c0, rows, off_y, in_h, got);
                                CHECK(got >= std::min(std::max(need + off_y, 0), in_h - 1), "fused=%d py=%d c0=%d rows=%d off_y=%d in_h=%d: waits for row %d, reads row %d", fused, py,
                                      c0, rows, off_y, in_h, got, need + off_y);
                            }
}

int main()
{
    test_tail16();
    test_tail32();
    test_tail32_frame();
    test_taper();
    test_first_chunk_last_row();
    std::printf(g_failed ? "%d properties FAILED\n" : "all cut properties hold\n", g_failed);
    return g_failed;
}
