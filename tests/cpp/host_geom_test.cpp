// host_geom_test.cpp -- the integers of the engine's host side (waifu2x-converter-cpp_amd/csrc/w2xc_host_geom.hpp) checked as properties on the CPU.
// Nothing here is taken from the code under test but the functions themselves: the conditions are what their consumers need --
//   * the units of a call tile its output rows, and a unit's source view holds every row its output rows read through the halo;
//   * the tapering first chunks make progress and end at whole slices;
//   * the runs of finished tile rows the drainer stitches tile a band's rows once;
//   * a job flag of an earlier band never reads as finished, up to and across the restart of the epochs;
//   * the sub-batches of a host batch cover its images once;
//   * the image pipeline's plane buffer holds every plane the batched pipeline lays out in it;
//   * the uint8 images of the RGBA call and its float planes lie in the declared order, each on a 256-byte boundary, none over another;
//   * the chroma planes of a YUV frame have the sizes the public header states, the device mirror of a host frame call keeps every plane of every frame
//     apart, and the float planes the frame pipelines carve are the ones the call reserved.
// Prints the first failing input of each property; exit status = number of failed properties.
#include "../../waifu2x-converter-cpp_amd/csrc/w2xc_host_geom.hpp"

#include <cstdio>

using namespace w2xc_eng;

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

// row counts around every threshold (8-row tiles, 16-row job rows, the slice sizes), the minimum sizes, the 1080 / 2160-row frames, 16384 rows
static std::vector<int> heights()
{
    std::vector<int> h;
    for (int r = 1; r <= 300; r++) h.push_back(r);
    const int more[] = {511, 512, 513, 1023, 1024, 1025, 1079, 1080, 1081, 2047, 2048, 2049, 2159, 2160, 2161, 4320, 16383, 16384};
    for (size_t i = 0; i < sizeof more / sizeof *more; i++) h.push_back(more[i]);
    return h;
}

// units tile [row_begin, row_end) in order; none is empty when nd <= R (convert_plane_host clamps nd to R)
static void test_unit_rows()
{
    const std::vector<int> hs = heights();
    for (size_t i = 0; i < hs.size(); i++)
        for (int row_begin = 0; row_begin <= 37; row_begin += 37)
            for (int nd = 1; nd <= 64 && nd <= hs[i]; nd++) {
                const int R = hs[i];
                int at = row_begin;
                for (int t = 0; t < nd; t++) {
                    const int ra = unit_rows(row_begin, row_begin + R, t, nd).first, rb = unit_rows(row_begin, row_begin + R, t, nd).second;
                    CHECK(ra == at && rb > ra, "R=%d row_begin=%d nd=%d: unit %d is [%d, %d), expected to start at %d", R, row_begin, nd, t, ra, rb, at);
                    at = rb;
                }
                CHECK(at == row_begin + R, "R=%d row_begin=%d nd=%d: units end at %d", R, row_begin, nd, at);
            }
}

// Output row y of the (h << up)-row plane reads rows y - hs .. y + hs of it, clipped to the plane (replicate border); row r of it is source row r >> up.
// A unit's source range [sy0, sy1) holds them all and lies inside the source plane, and so does what a band that ends at y1 has uploaded.
static void test_src_rows()
{
    const std::vector<int> hv = heights();
    const int halos[] = {1, 3, 7, 28};
    for (int up = 0; up <= 1; up++)
        for (size_t i = 0; i < hv.size(); i++)
            for (size_t k = 0; k < sizeof halos / sizeof *halos; k++) {
                const int h = hv[i], H = h << up, hs = halos[k];
                const int cuts[] = {0, 1, hs, hs + 1, H / 3, H / 2, H / 2 + 1, H - hs - 1, H - hs, H - 1, H};
                for (size_t a = 0; a < sizeof cuts / sizeof *cuts; a++)
                    for (size_t b = 0; b < sizeof cuts / sizeof *cuts; b++) {
                        const int ra = cuts[a], rb = cuts[b];
                        if (ra < 0 || rb > H || ra >= rb) continue;
                        const int sy0 = src_rows(ra, rb, hs, up, H).first, sy1 = src_rows(ra, rb, hs, up, H).second;
                        CHECK(0 <= sy0 && sy0 < sy1 && sy1 <= h, "up=%d h=%d hs=%d [%d, %d): source rows [%d, %d) outside the plane", up, h, hs, ra, rb, sy0, sy1);
                        const int first = std::max(0, ra - hs) >> up, last = std::min(H - 1, rb - 1 + hs) >> up;
                        CHECK(sy0 <= first && last < sy1, "up=%d h=%d hs=%d [%d, %d): reads source rows %d..%d, has [%d, %d)", up, h, hs, ra, rb, first, last, sy0, sy1);
                        for (int y1 = ra + 1; y1 <= rb; y1 += (y1 < ra + 40 || y1 > rb - 40) ? 1 : 97) {
                            const int end = band_src_end(y1, hs, up, H, sy0, false, sy1 - sy0), need = (std::min(H - 1, y1 - 1 + hs) >> up) - sy0;
                            CHECK(need < end && end <= sy1 - sy0, "up=%d h=%d hs=%d [%d, %d): a band that ends at %d reads view row %d, %d uploaded of %d", up, h, hs, ra, rb,
                                  y1, need, end, sy1 - sy0);
                        }
                        CHECK(band_src_end(ra + 1, hs, up, H, sy0, true, sy1 - sy0) == sy1 - sy0, "up=%d h=%d hs=%d: overlapping planes stage the whole view first", up, h, hs);
                    }
            }
}

// the staging sizes are whole rows, at least one (eight for the output: the last-layer kernels' tiles), the taper's minimum is not above its maximum;
// tapering chunks are positive and, from any start, reach a whole slice and stay there
static void test_chunks()
{
    const int kbs[] = {0, 1, 4, 16, 64, 1024, 8192, 65536}, widths[] = {1, 4, 31, 256, 1920, 3840, 7680, 1 << 20};
    for (size_t a = 0; a < sizeof kbs / sizeof *kbs; a++)
        for (size_t b = 0; b < sizeof widths / sizeof *widths; b++)
            for (int up = 0; up <= 1; up++) {
                const int kb = kbs[a], w = widths[b];
                const HostChunks c = host_chunks(kb, (size_t)w * 4, (size_t)(w << up) * 4);
                CHECK(c.in_rows >= 1 && c.out_rows >= 8 && c.out_min >= 8, "kb=%d w=%d up=%d: chunks of %d / %d / %d rows", kb, w, up, c.in_rows, c.out_rows, c.out_min);
                CHECK(c.out_rows % 8 == 0 && c.out_min % 8 == 0 && c.out_min <= c.out_rows, "kb=%d w=%d up=%d: output chunks of %d tapering to %d rows", kb, w, up, c.out_rows, c.out_min);
                const int full = layer1_chunk(c.in_rows, up);
                CHECK(full >= 8 && full % 8 == 0 && full >= (c.in_rows << up), "kb=%d w=%d up=%d: layer-1 chunks of %d rows for slices of %d", kb, w, up, full, c.in_rows);
                for (int start = 0; start <= 2 * full; start += std::max(1, full / 37)) {
                    int c0 = start, steps = 0;
                    bool at_full = false;
                    for (; steps < 64; steps++) {
                        const int rows = taper_chunk(c0, full);
                        CHECK(rows > 0 && rows <= full, "full=%d c0=%d: chunk of %d rows", full, c0, rows);
                        CHECK(!at_full || rows == full, "full=%d c0=%d: %d rows after a whole slice", full, c0, rows);
                        at_full = rows == full;
                        c0 += rows;
                    }
                    CHECK(at_full, "full=%d start=%d: no whole slice after %d chunks", full, start, steps);
                }
            }
}

// job row jr of a band of R rows holds rows [16 jr - first, 16 jr - first + 16) clipped: trows = ceil((R + first) / 16) job rows.  However the finished
// job rows come in -- one by one, in runs, all at once -- the spans stitched tile [0, R) in order, nothing twice
static void test_tile_rows_span()
{
    const std::vector<int> hv = heights();
    const int strides[] = {1, 2, 3, 7, 1 << 20};
    for (size_t i = 0; i < hv.size(); i++)
        for (int first = 0; first <= 15; first++)
            for (size_t s = 0; s < sizeof strides / sizeof *strides; s++) {
                const int R = hv[i], trows = (R + first + 15) / 16;
                int at = 0;
                for (int jr = 0; jr < trows;) {
                    const int ready = std::min(trows, jr + strides[s]);
                    const int a = tile_rows_span(jr, ready, first, R).first, b = tile_rows_span(jr, ready, first, R).second;
                    if (b > a) {
                        CHECK(a == at && b <= R, "R=%d first=%d: job rows [%d, %d) cover [%d, %d), stitched so far %d", R, first, jr, ready, a, b, at);
                        at = b;
                    }
                    jr = ready;
                }
                CHECK(at == R, "R=%d first=%d stride=%d: rows stitched end at %d", R, first, strides[s], at);
            }
}

// A band's jobs store its epoch; the words hold 0 (fresh) or the epoch of any earlier band since.  Only the current band's value may read as finished,
// for the first bands of a buffer and for the last ones before PROG_EPOCH_LAST, where the flags are zeroed and the epochs start over.
static void test_flag_epochs()
{
    const unsigned starts[] = {0u, 1u, 1000u, 0x3FFFFFFFu, 0x7FFFFFF0u};
    for (size_t s = 0; s < sizeof starts / sizeof *starts; s++) {
        unsigned epoch = starts[s];
        std::vector<unsigned> words;   // every value a flag can still hold
        words.push_back(0);
        if (epoch > 0) { words.push_back(1); words.push_back(epoch / 2 + 1); words.push_back(epoch); }
        for (int band = 0; band < 40; band++) {
            if (epoch == PROG_EPOCH_LAST) { words.assign(1, 0u); epoch = 0; }   // (what prog_begin does)
            const unsigned e = ++epoch;
            CHECK(e >= 1 && e <= PROG_EPOCH_LAST, "epoch %u handed out", e);
            for (size_t k = 0; k < words.size(); k++) CHECK(!flag_reached(words[k], e), "a flag that holds %u reads as finished in epoch %u", words[k], e);
            CHECK(flag_reached(e, e), "a flag that holds %u does not read as finished in its own epoch", e);
            words.push_back(e);
        }
    }
    // The test is the SIGNED distance flag - epoch, not flag >= epoch: it holds for flags up to 2^31 - 1 behind their epoch and no further.  That is why the
    // epochs may not run past PROG_EPOCH_LAST: at PROG_EPOCH_LAST + 1 a fresh (zero) flag still reads as unfinished, one epoch later it would read as finished.
    CHECK(!flag_reached(0u, PROG_EPOCH_LAST + 1u), "a fresh flag reads as finished in epoch 2^31");
    CHECK(flag_reached(0u, PROG_EPOCH_LAST + 2u), "the flag test is not the signed distance: a flag 2^31 - 1 ahead (mod 2^32) does not read as finished");
    CHECK(flag_reached(5u, 0xFFFFFFFEu) && !flag_reached(0xFFFFFFFEu, 5u), "the flag test is not the signed distance across the 2^32 wrap");
}

// the sub-batches of n images cover 0 .. n once, in order on every device, each of 1 .. sub images, on no more devices than there are
static void test_batch_stripes()
{
    const int ns[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 64, 100, 255, 1000, 4097}, subs[] = {1, 2, 3, 8, 33, 64, 1 << 20};
    for (size_t a = 0; a < sizeof ns / sizeof *ns; a++)
        for (size_t b = 0; b < sizeof subs / sizeof *subs; b++)
            for (int ndev = 1; ndev <= 8; ndev++) {
                const int n = ns[a], sub = batch_stripe_sub(subs[b], n, ndev);
                CHECK(sub >= 1 && sub <= subs[b], "n=%d sub=%d ndev=%d: sub-batches of %d", n, subs[b], ndev, sub);
                const std::vector<std::vector<std::pair<int, int> > > share = batch_stripes(n, sub, ndev);
                CHECK(!share.empty() && (int)share.size() <= ndev, "n=%d sub=%d ndev=%d: %d shares", n, sub, ndev, (int)share.size());
                std::vector<int> seen(n, 0);
                for (size_t d = 0; d < share.size(); d++) {
                    CHECK(!share[d].empty(), "n=%d sub=%d ndev=%d: device %d has nothing to do", n, sub, ndev, (int)d);
                    int prev_end = -1;
                    for (size_t j = 0; j < share[d].size(); j++) {
                        const int first = share[d][j].first, cnt = share[d][j].second;
                        CHECK(cnt >= 1 && cnt <= sub && first >= 0 && first + cnt <= n, "n=%d sub=%d ndev=%d: sub-batch [%d, +%d)", n, sub, ndev, first, cnt);
                        CHECK(first >= prev_end, "n=%d sub=%d ndev=%d: device %d's sub-batches out of order at image %d", n, sub, ndev, (int)d, first);
                        prev_end = first + cnt;
                        for (int i = first; i < first + cnt; i++) seen[i]++;
                    }
                }
                for (int i = 0; i < n; i++) CHECK(seen[i] == 1, "n=%d sub=%d ndev=%d: image %d is in %d sub-batches", n, sub, ndev, i, seen[i]);
            }
}

// The Y image pipeline lays its planes out per level, `cap` images wide (S <= cap of them in use), every plane on a 256-byte boundary: level 0 holds
// Y, U, V and the noise pass's second Y; every scale iteration Y, U, V of twice the size; the shrink Y, U, V of the final size.  All of it lies inside
// cap x image_aux_floats, and no level runs into the next.  With alpha (the RGBA call: one image) every Y is a group of two planes, Y and its alpha --
// on level 0 twice, in every level and in the shrink -- and U follows the group.
static void test_image_aux()
{
    const int sizes[][2] = {{1, 1}, {3, 5}, {7, 9}, {8, 8}, {63, 1}, {64, 64}, {65, 63}, {256, 256}, {640, 480}, {1920, 1080}};
    const double shrinks[] = {0.0, 0.3, 0.5, 0.99};
    for (size_t i = 0; i < sizeof sizes / sizeof *sizes; i++)
        for (int it = 0; it <= 4; it++)
            for (size_t k = 0; k < sizeof shrinks / sizeof *shrinks; k++)
                for (int cap = 1; cap <= 33; cap += 16)
                    for (int S = 1; S <= cap; S += cap - 1 > 0 ? cap - 1 : 1)
                      for (int alpha = 0; alpha <= (cap == 1 ? 1 : 0); alpha++) {
                        const size_t ya = alpha ? 2 : 1, ny = ya * (size_t)S;   // planes of a Y, of the Y group
                        const int w = sizes[i][0], h = sizes[i][1];
                        const double shrink = shrinks[k];
                        int fw, fh;
                        final_size(w, h, it, shrink, &fw, &fh);
                        if (fw < 1 || fh < 1) continue;   // (refused by the argument checks)
                        CHECK(fw <= (w << it) && fh <= (h << it), "%dx%d it=%d shrink=%g: final size %dx%d", w, h, it, shrink, fw, fh);
                        const size_t have = image_aux_floats(w, h, it, shrink, alpha != 0) * (size_t)cap;
                        size_t base = 0, end = 0;
                        // planes [first, first + count) of a level whose planes are ps floats apart hold cw x ch floats each
                        struct { size_t *end; bool ok; void use(size_t base, size_t ps, size_t first, size_t count, size_t px) {
                            ok = ok && px <= ps && ps % 64 == 0;
                            *end = std::max(*end, base + (first + count - 1) * ps + px); } } lay = {&end, true};
                        int cw = w, ch = h;
                        size_t ps = plane_floats(cw, ch);
                        lay.use(base, ps, 0, ny, (size_t)cw * ch);                        // the Y group
                        lay.use(base, ps, ny, 2 * (size_t)S, (size_t)cw * ch);           // u, v: S planes each
                        lay.use(base, ps, ny + 2 * (size_t)S, ny, (size_t)cw * ch);      // the noise pass's Y group
                        base += (2 * ya + 2) * (size_t)cap * ps;
                        CHECK(end <= base, "%dx%d it=%d cap=%d S=%d: level 0 runs into the next level", w, h, it, cap, S);
                        for (int l = 0; l < it; l++) {
                            cw *= 2; ch *= 2;
                            ps = plane_floats(cw, ch);
                            lay.use(base, ps, 0, ny + 2 * (size_t)S, (size_t)cw * ch);   // the Y group, then u, v
                            base += (ya + 2) * (size_t)cap * ps;
                            CHECK(end <= base, "%dx%d it=%d cap=%d S=%d: level %d runs into the next level", w, h, it, cap, S, l + 1);
                        }
                        if (shrink > 0.0) lay.use(base, plane_floats(fw, fh), 0, ny + 2 * (size_t)S, (size_t)fw * fh);
                        CHECK(lay.ok, "%dx%d it=%d: a plane is larger than its slot or not on a 256-byte boundary", w, h, it);
                        CHECK(end <= have, "%dx%d it=%d shrink=%g cap=%d S=%d alpha=%d: planes end at float %zu, the buffer holds %zu", w, h, it, shrink, cap, S, alpha, end, have);
                      }
}

// the sweep of the RGBA and YUV layouts: odd and even sides, below, at and above a 64-float plane boundary, mixed across w and h
static const int kSides[] = {1, 2, 3, 17, 64, 65};
static const int kNSides = sizeof kSides / sizeof *kSides;

// The RGBA call keeps five kinds of uint8 images and its float planes in one buffer, cap images of each kind side by side (plan_rgba gives the bytes per image:
// multiples of 256, 0 where the call has none).  Each region starts on a 256-byte boundary, directly behind the one before it in the declared order -- so none
// lies over another and an absent one takes no room -- and the buffer ends where the float planes do.
static void test_rgba_layout()
{
    for (int a = 0; a < kNSides; a++)
        for (int b = 0; b < kNSides; b++)
            for (int cap = 1; cap <= 3; cap += 2)
                for (int it = 0; it <= 1; it++)
                    for (int mask = 0; mask < 32; mask++) {
                        const int w = kSides[a], h = kSides[b], fw = w << it, fh = h << it;
                        RgbaImageBytes R;
                        const size_t src3 = align256((size_t)w * 3 * h), dst3 = align256((size_t)fw * 3 * fh);
                        R.bled = mask & 1 ? src3 : 0; R.stamp = mask & 2 ? align256((size_t)w * 2 * h) : 0; R.res = mask & 4 ? dst3 : 0;
                        R.grey = mask & 8 ? src3 : 0; R.ares = mask & 16 ? dst3 : 0;
                        R.floats = image_aux_floats(w, h, it, 0.0, it != 0);
                        const RgbaLayout L(R, (size_t)cap);
                        const size_t off[] = {L.bled, L.stamp, L.res, L.grey, L.ares, L.head}, img[] = {R.bled, R.stamp, R.res, R.grey, R.ares};
                        CHECK(off[0] == 0, "%dx%d cap=%d mask=%d: the first region starts at %zu", w, h, cap, mask, off[0]);
                        for (int k = 0; k < 5; k++) {
                            CHECK(off[k] % 256 == 0 && off[k + 1] % 256 == 0, "%dx%d cap=%d mask=%d: region %d starts at %zu, the next at %zu", w, h, cap, mask, k, off[k], off[k + 1]);
                            CHECK(off[k + 1] == off[k] + (size_t)cap * img[k], "%dx%d cap=%d mask=%d: region %d [%zu, +%d x %zu) and the next at %zu", w, h, cap, mask, k, off[k],
                                  cap, img[k], off[k + 1]);
                        }
                        CHECK(L.bytes == L.head + (size_t)cap * R.floats * sizeof(float), "%dx%d cap=%d mask=%d: %zu bytes, the float planes end at %zu", w, h, cap, mask, L.bytes,
                              L.head + (size_t)cap * R.floats * sizeof(float));
                    }
}

// The chroma planes of a w x h frame are ceil(w / 2) x ceil(h / 2) (4:2:0), ceil(w / 2) x h (4:2:2), w x h (4:4:4), none (4:0:0) -- include/w2xc_hip.h.
// The device mirror of one side of a host frame call holds cap frames: all luma planes, then all chroma -- planar U and V, or the two interleaved planes as ONE
// plane of 2 cw-byte rows in which U and V are neighbouring bytes.  No plane of any frame touches another, every frame of luma and of chroma starts on a
// 256-byte boundary, a frame stride covers the frame, the planes hold yuv_frame_bytes samples per frame, and the total -- what img_io.reserve is given -- is
// where the last plane's 256-byte share ends.
static void test_yuv_mirror()
{
    const int layouts[] = {W2XC_YUV_420, W2XC_YUV_422, W2XC_YUV_444, W2XC_YUV_400};
    for (int a = 0; a < kNSides; a++)
        for (int b = 0; b < kNSides; b++)
            for (int li = 0; li < 4; li++)
                for (int c_px = 1; c_px <= 2; c_px++)
                    for (int u_first = 0; u_first <= 1; u_first++)
                        for (int cap = 1; cap <= 3; cap += 2) {
                            const int w = kSides[a], h = kSides[b], chroma = layouts[li];
                            const ChromaSize cs = yuv_chroma_size(w, h, chroma);
                            const int want_cw = chroma == W2XC_YUV_400 ? 0 : chroma == W2XC_YUV_444 ? w : w / 2 + w % 2;
                            const int want_ch = chroma == W2XC_YUV_400 ? 0 : chroma == W2XC_YUV_420 ? h / 2 + h % 2 : h;
                            CHECK(cs.cw == want_cw && cs.ch == want_ch, "%dx%d layout %d: chroma planes of %dx%d, the header says %dx%d", w, h, chroma, cs.cw, cs.ch, want_cw, want_ch);
                            const YuvMirrorLayout m = yuv_mirror_layout(c_px, u_first != 0, cap, w, h, cs.cw, cs.ch);
                            // [start, end) of every plane of every frame, and the samples they hold
                            std::vector<std::pair<size_t, size_t> > planes;
                            size_t samples = 0;
                            CHECK(m.y_stride >= (size_t)w, "%dx%d: luma rows %zu bytes apart", w, h, m.y_stride);
                            const size_t y_ext = (size_t)(h - 1) * m.y_stride + w;
                            CHECK(m.y_frame_stride >= y_ext && m.y_frame_stride % 256 == 0, "%dx%d: luma frames %zu bytes apart, a plane takes %zu", w, h, m.y_frame_stride, y_ext);
                            for (int i = 0; i < cap; i++) planes.push_back(std::make_pair(i * m.y_frame_stride, i * m.y_frame_stride + y_ext));
                            samples += (size_t)w * h;
                            if (cs.cw) {
                                const size_t first = std::min(m.u, m.v), row = m.pair ? 2 * (size_t)cs.cw : (size_t)cs.cw, c_ext = (size_t)(cs.ch - 1) * m.c_stride + row;
                                CHECK(m.pair == (c_px == 2) && m.c_copy_row == row && m.c_stride >= row, "%dx%d layout %d c_px=%d: chroma rows of %zu bytes, %zu apart, copied %zu at a time",
                                      w, h, chroma, c_px, row, m.c_stride, m.c_copy_row);
                                CHECK(first % 256 == 0 && m.c_frame_stride % 256 == 0, "%dx%d layout %d c_px=%d: chroma frames start at %zu + i * %zu", w, h, chroma, c_px, first, m.c_frame_stride);
                                // a plane as the kernels address it -- samples c_px bytes apart -- lies inside the rows the copies move
                                CHECK(chroma_row_bytes(cs.cw, c_px) <= row, "%dx%d layout %d c_px=%d: a row of %zu bytes in rows of %zu", w, h, chroma, c_px, chroma_row_bytes(cs.cw, c_px), row);
                                if (m.pair) {
                                    CHECK(m.c_stride == 2 * (size_t)cs.cw, "%dx%d layout %d: interleaved rows %zu bytes apart, 2 cw = %d", w, h, chroma, m.c_stride, 2 * cs.cw);
                                    CHECK(u_first ? m.v == m.u + 1 : m.u == m.v + 1, "%dx%d layout %d u_first=%d: U at %zu, V at %zu", w, h, chroma, u_first, m.u, m.v);
                                    CHECK(m.c_frame_stride >= c_ext, "%dx%d layout %d: interleaved frames %zu apart, a plane takes %zu", w, h, chroma, m.c_frame_stride, c_ext);
                                    for (int i = 0; i < cap; i++) planes.push_back(std::make_pair(first + i * m.c_frame_stride, first + i * m.c_frame_stride + c_ext));
                                } else {
                                    CHECK(m.c_frame_stride >= std::max(m.u, m.v) - first + c_ext, "%dx%d layout %d: planar frames %zu apart, U and V take %zu", w, h, chroma,
                                          m.c_frame_stride, std::max(m.u, m.v) - first + c_ext);
                                    for (int i = 0; i < cap; i++) {
                                        planes.push_back(std::make_pair(m.u + i * m.c_frame_stride, m.u + i * m.c_frame_stride + c_ext));
                                        planes.push_back(std::make_pair(m.v + i * m.c_frame_stride, m.v + i * m.c_frame_stride + c_ext));
                                    }
                                }
                                samples += 2 * (size_t)cs.cw * cs.ch;
                            } else CHECK(m.c_copy_row == 0, "%dx%d layout %d: no chroma, but rows of %zu bytes to copy", w, h, chroma, m.c_copy_row);
                            CHECK(samples == yuv_frame_bytes(w, h, cs.cw, cs.ch), "%dx%d layout %d: the planes hold %zu samples, yuv_frame_bytes says %zu", w, h, chroma, samples,
                                  yuv_frame_bytes(w, h, cs.cw, cs.ch));
                            std::sort(planes.begin(), planes.end());
                            for (size_t k = 1; k < planes.size(); k++)
                                CHECK(planes[k - 1].second <= planes[k].first, "%dx%d layout %d c_px=%d cap=%d: the plane at %zu runs to %zu, into the one at %zu", w, h, chroma, c_px, cap,
                                      planes[k - 1].first, planes[k - 1].second, planes[k].first);
                            const size_t end = planes.back().second;
                            CHECK(m.bytes >= end && m.bytes == align256(end), "%dx%d layout %d c_px=%d cap=%d: %zu bytes, the last plane ends at %zu", w, h, chroma, c_px, cap, m.bytes, end);
                        }
}

// The float planes the frame pipelines carve per frame, walked level by level, against what the calls reserve per frame.
//   process_yuv_device      level 0: the luma plane and the noise pass's output; with a scale pass ONE plane of the doubled size.  yuv_aux_floats reserves two
//                           planes on every level, so with a scale pass exactly one plane of the doubled size stays unused.
//   process_yuv_rgb_device  level 0: R, G, B; the noise pass's three output planes on the same level; a scale pass's three of the doubled size.  yuv_rgb_aux_floats
//                           is their sum.
static void test_yuv_aux()
{
    for (int a = 0; a < kNSides; a++)
        for (int b = 0; b < kNSides; b++)
            for (int it = 0; it <= 1; it++)
                for (int noise = 0; noise <= 1; noise++) {
                    const int w = kSides[a], h = kSides[b];
                    size_t y_carved = 2 * plane_floats(w, h), rgb_carved = 3 * plane_floats(w, h);
                    if (noise) rgb_carved += 3 * plane_floats(w, h);
                    int lw = w, lh = h;
                    for (int l = 0; l < it; l++) {
                        lw *= 2; lh *= 2;
                        y_carved += plane_floats(lw, lh);
                        rgb_carved += 3 * plane_floats(lw, lh);
                    }
                    const size_t spare = it ? plane_floats(2 * w, 2 * h) : 0;
                    CHECK(yuv_aux_floats(w, h, it) == y_carved + spare, "%dx%d it=%d: the Y call reserves %zu floats per frame, carves %zu and leaves %zu", w, h, it,
                          yuv_aux_floats(w, h, it), y_carved, spare);
                    CHECK(yuv_rgb_aux_floats(noise != 0, w, h, it) == rgb_carved, "%dx%d it=%d noise=%d: the RGB call reserves %zu floats per frame, carves %zu", w, h, it, noise,
                          yuv_rgb_aux_floats(noise != 0, w, h, it), rgb_carved);
                }
}

// The launch grid of the YUV tile kernels: chroma2x_tile_grid / yuv_rgb_tile_grid against the expressions the six launchers each wrote out before the rule had one
// home -- tile counts, tiles, turns (n * npl per tile for the 8-bit chroma kernel, n for the 16-bit one and the four of the RGB route) and the capped grid.
static void test_yuv_tile_grid()
{
    const int TX = 32, TY = 16;   // W2XC_CHROMA_TQX / _TQY and W2XC_YUVRGB_TCX / _TCY
    const long long CAP = 2048;   // W2XC_CHROMA_GRID_MAX and W2XC_YUVRGB_GRID_MAX
    const int sizes[] = {1, 31, 32, 33, 63, 64, 65};
    const int ns[] = {1, 3};
    for (int w : sizes)
        for (int h : sizes)
            for (int n : ns)
                for (int npl = 1; npl <= 2; npl++) {
                    {   // w2xc_launch_chroma2x_u8 (per_tile = n * npl) and w2xc_launch_chroma2x_u16 (per_tile = n), w x h the OUTPUT
                        const int tiles_x = (w / 2 + TX) / TX, tiles_y = (h / 2 + TY) / TY;
                        const long long tiles = (long long)tiles_x * tiles_y;
                        for (long long per : {(long long)n * npl, (long long)n}) {
                            const long long turns = tiles * per;
                            const unsigned grid = (unsigned)(turns > CAP ? CAP : turns);
                            const YuvTileGrid g = chroma2x_tile_grid(w, h, per, TX, TY, CAP);
                            CHECK(g.tiles_x == tiles_x && g.tiles == tiles && g.turns == turns && g.grid == grid, "chroma 2x %dx%d per_tile=%lld: %d %lld %lld %u", w, h, per,
                                  g.tiles_x, g.tiles, g.turns, g.grid);
                        }
                    }
                    {   // the four launchers of the RGB route, w x h the CHROMA plane
                        const int tiles_x = (w + TX - 1) / TX, tiles_y = (h + TY - 1) / TY;
                        const long long tiles = (long long)tiles_x * tiles_y, turns = tiles * n;
                        const unsigned grid = (unsigned)(turns > CAP ? CAP : turns);
                        const YuvTileGrid g = yuv_rgb_tile_grid(w, h, n, TX, TY, CAP);
                        CHECK(g.tiles_x == tiles_x && g.tiles == tiles && g.turns == turns && g.grid == grid, "rgb route %dx%d n=%d: %d %lld %lld %u", w, h, n, g.tiles_x,
                              g.tiles, g.turns, g.grid);
                    }
                }
    // more turns than workgroups: the cap holds, the turns do not shrink
    const YuvTileGrid c = chroma2x_tile_grid(1920, 1080, 16, TX, TY, CAP), r = yuv_rgb_tile_grid(960, 540, 8, TX, TY, CAP);
    CHECK(c.tiles_x == 31 && c.tiles == 31 * 34 && c.turns == 31 * 34 * 16 && c.grid == 2048, "chroma 2x above the cap: %d %lld %lld %u", c.tiles_x, c.tiles, c.turns, c.grid);
    CHECK(r.tiles_x == 30 && r.tiles == 30 * 34 && r.turns == 30 * 34 * 8 && r.grid == 2048, "rgb route above the cap: %d %lld %lld %u", r.tiles_x, r.tiles, r.turns, r.grid);
    const YuvTileGrid edge = yuv_tile_grid(1, 2049, 1, CAP), at = yuv_tile_grid(1, 2048, 1, CAP);
    CHECK(edge.turns == 2049 && edge.grid == 2048 && at.turns == 2048 && at.grid == 2048, "the cap at 2048 / 2049 turns: %u %u", at.grid, edge.grid);
}

int main()
{
    test_yuv_tile_grid();
    test_unit_rows();
    test_src_rows();
    test_chunks();
    test_tile_rows_span();
    test_flag_epochs();
    test_batch_stripes();
    test_image_aux();
    test_rgba_layout();
    test_yuv_mirror();
    test_yuv_aux();
    std::printf(g_failed ? "%d properties FAILED\n" : "all host geometry properties hold\n", g_failed);
    return g_failed;
}
