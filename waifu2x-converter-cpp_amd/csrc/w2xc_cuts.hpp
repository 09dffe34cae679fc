// w2xc_cuts.hpp -- where the chunked launch strategies of w2xc_rows.cpp cut a band's rows.  Pure integer arithmetic: no HIP, no engine type, so that
// tests/cpp/cuts_test.cpp checks it on the CPU.  Rows are LOCAL to the launch's region / the band; a callback that returns non-zero ends the walk with that value.
#pragma once
#include <algorithm>
#include <cstdlib>

namespace w2xc_eng {

// 16-bit tail (tail16): layer n - 1 and the gather TOGETHER in row chunks (quarters of the band's R rows, whole 16-row tiles): chunk j's rows leave for the
// host under layer n - 1 of chunk j + 1.  The producer chunks tile the G rows [0, R + 2) without overlap (chunk j computes G rows up to r1 + 2, the next one
// continues there): no recompute.  producer(g0, g1) = one launch of layer n - 1 for G rows [g0, g1); piece(a, b) = one gather of output rows [a, b).
template <class P, class G> int cut_tail16(int R, P &&producer, G &&piece)
{
    const int cr = std::max(64, ((R / 4) + 15) & ~15);
    int g_done = 0;
    for (int r0 = 0; r0 < R;) {
        int r1 = std::min(R, r0 + cr);
        if (R - r1 < 32) r1 = R;
        const int g1 = r1 + 2;                       // the gather of rows [r0, r1) reads G rows [r0, r1 + 2)
        if (int rc = producer(g_done, g1)) return rc;
        g_done = g1;
        // the gather of the chunk's rows; the LAST chunk's gather in pieces of ~128 rows, each handed to the download as soon as it
        // is enqueued: what nothing can hide is then the download + stitch of the last ~2 MB piece, not of the whole last chunk
        const int step = (r1 == R && r1 - r0 > 192) ? 128 : r1 - r0;
        for (int a = r0; a < r1;) {
            int b = std::min(r1, a + step);
            if (r1 - b < 64) b = r1;
            if (int rc = piece(a, b)) return rc;
            a = b;
        }
        r0 = r1;
    }
    return 0;
}

// ... a launch whose item count is not a multiple of the 256 persistent workgroups ends with a partly filled round: among the tile-row
// counts within 8 of the wanted one, take the one that wastes the fewest workgroup slots (2160x3840, two 64-plane blocks: 64 + 48 + 24
// tile rows = 60 + 45 + 22.5 rounds against 63.75 + 40.3 + 23.4 for exact halves)
inline int chunk_rows(int want, int items_per_row)
{
    int best = std::max(4, (want + 15) / 16), waste = 1 << 30;
    for (int r = std::max(4, (want + 15) / 16 - 8); r <= (want + 15) / 16 + 8; r++) {
        const int items = items_per_row * r, w_ = ((items + 255) / 256) * 256 - items;
        if (w_ < waste || (w_ == waste && std::abs(r * 16 - want) < std::abs(best * 16 - want))) { waste = w_; best = r; }
    }
    return best * 16;
}

// fp32 tail (tail32): the producer's RL region rows in three launches -- 1/2, then 5/16, then the rest -- of whole 16-row tiles: every launch of the persistent
// kernel has a ramp and a tail (measured: four equal chunks cost layer 6 +0.6 ms on the 2160x3840 frame), while what the LAST chunk writes cannot hide behind
// compute.  The last layer's R output rows follow two rows behind: output row y reads producer rows y + off_l .. y + off_l + 2.
// producer(p0, p1) = one launch of layer n - 1 for its rows [p0, p1); piece(a, b) = one launch of the last layer for output rows [a, b).
template <class P, class G> int cut_tail32(int RL, int R, int off_l, int items_per_row, P &&producer, G &&piece)
{
    for (int p0 = 0, o0 = 0, ci = 0; p0 < RL; ci++) {
        const int want = ci == 0 ? RL / 2 : ci == 1 ? (RL * 5) / 16 : RL;
        int p1 = ci < 2 ? std::min(RL, p0 + chunk_rows(want, items_per_row)) : RL;
        if (RL - p1 < 64) p1 = RL;
        if (int rc = producer(p0, p1)) return rc;
        const int o1 = p1 == RL ? R : std::min(R, std::max(o0, p1 - off_l - 2));   // output rows whose three input rows exist
        // the LAST chunk's rows in pieces of ~128, its last 128 in pieces of 64: what nothing can hide is then the download + stitch of the last piece only
        const int step = (p1 == RL && o1 - o0 > 192) ? 128 : std::max(o1 - o0, 1);
        for (int a = o0; a < o1;) {
            int b = std::min(o1, a + ((p1 == RL && o1 - a <= 160 && o1 - a > 96) ? 64 : step));
            if (o1 - b < 48) b = o1;
            if (int rc = piece(a, b)) return rc;
            a = b;
        }
        p0 = p1;
        o0 = o1;
    }
    return 0;
}

// the last layer's out_h rows in chunks: a third of what is left, within [min, max], in whole 8-row tiles: big chunks while there is compute
// left to hide their D2H behind, small ones at the end where the D2H is exposed.  chunk(c0, rows).
template <class F> int cut_taper(int out_h, int max_rows, int min_rows, F &&chunk)
{
    const int lo = std::max(min_rows, 8);
    for (int c0 = 0, cr = 0; c0 < out_h; c0 += cr) {
        const int left = out_h - c0;
        cr = std::min(max_rows, std::max(lo, ((left / 3) + 7) & ~7));
        if (left - cr < lo) cr = left;
        if (int rc = chunk(c0, cr)) return rc;
    }
    return 0;
}

// last VIEW row a first-layer chunk of output rows [c0, c0 + rows) reads.  Layer 1 alone: its last row + 2.  The fused launch (layers 1 + 2): the chunk ends
// on a multiple of 8 LOCAL rows, which is a 4x4-block edge only when wino_py = 0; the block that straddles the end reads its whole 6-row patch -- every row of
// it enters every output row of the block at rounding level (and as NaN if the row holds one) -- so the wait covers the last TOUCHED block: its last row + 4
inline int first_chunk_last_row(int c0, int rows, bool fused, int wino_py, int off_y, int in_h)
{
    int last = c0 + rows - 1 + 2;
    if (fused) last = (((c0 + rows + wino_py + 3) & ~3) - wino_py) - 1 + 4;
    return std::min(std::max(last + off_y, 0), in_h - 1);
}

}  // namespace w2xc_eng
