// w2xc_wino4_body.inc -- the body of conv3x3_wino4 (w2xc_wino4.hip; the design notes are there), included by the one-image kernel and by its batch form
// conv3x3_wino4_batch.  The includer defines the batch hooks:
//   W4B_ONLY(...)      the batch form's own statements (nothing in the one-image kernel)
//   W4B_SEL(b, s)      b in the batch form, s in the one-image kernel
//   W4B_OUT            the output base of the epilogue's item: d.out, or the item's image's (d.out + image x bd.out_bs)
// so that the one-image kernel's text -- and its instruction stream -- is exactly that of round 6.  Batch: `nitems` = batch x bd.items items, image-major;
// an item decodes to (image, tile, 64-plane block), and the image moves only the scalar bases of the input tile and of the epilogue's stores.
    static_assert(!PROG || FUSE7, "PROG finishes the fused last layer");
    constexpr int ROWS = 16;
    constexpr int NST = CIN / 4;                            // stages (4-channel slices) per item
    constexpr int NOB = COUT / 64;                          // 64-plane blocks
    constexpr int CHS = 168;                                // chunks per channel of a raw buffer (18 rows x 9 quads = 162, + 6: stride = 8 mod 16)
    constexpr int RAW_PIECES = 11;                          // 4 x 168 = 672 chunks = 10.5 pieces of 64 x 16 bytes
    constexpr unsigned RAW_BYTES = RAW_PIECES * 1024;
    constexpr unsigned U_BASE = 3 * RAW_BYTES, U_BYTES = 36 * 1024;
    constexpr unsigned V_BASE = U_BASE + 2 * U_BYTES, V_BYTES = 18 * 1024;
    constexpr unsigned SPARE_BASE = V_BASE + 2 * V_BYTES;   // 18 KiB: with U slot 1 and V slot 1 the fused last layer's exchange across an epilogue (PARK: with U slot 1 the parking area)
    constexpr unsigned BIAS_BASE = SPARE_BASE + V_BYTES;
    static_assert(CIN % 16 == 0 && COUT % 64 == 0 && NST % 4 == 0 && NST >= 8, "planes");
    constexpr int STRIP = 16;
    constexpr int GW = 8;                                   // PROG: tiles per gather-job column group
    constexpr unsigned TRIG_BASE = BIAS_BASE + COUT * 4;    // PROG: one LDS word, the jobs this workgroup's arrivals completed
    const int tiles_y = W4B_SEL(bd.items, nitems) / (NOB * tiles_x);
    W4B_ONLY(const int img_tiles = bd.items / NOB;)   // (batch: tiles per image)
    const int pxcd = blockIdx.x & 7;
    auto band_lo = [&](int k, int r) { return (k * tiles_x + (r & 7)) >> 3; };   // PROG: first tile column of XCD k in tile row r
    auto tile_coords = [&](int pt_, int &ty_, int &tx_) {     // strips of 16 tiles, row by row inside a strip (the next round of an XCD is the tile row below)
        W4B_ONLY(pt_ = pt_ % img_tiles;)                      // (batch: the tile inside its image)
        if constexpr (PROG) {   // pt_ = index into THIS XCD's band, row by row; a period of eight rows holds exactly tiles_x of its tiles
            const int p8 = pt_ / tiles_x;
            int rem = pt_ - p8 * tiles_x, j = 0, lo = band_lo(pxcd, 0), wd = band_lo(pxcd + 1, 0) - lo;
            while (rem >= wd && j < 7) {
                rem -= wd;
                j++;
                lo = band_lo(pxcd, j);
                wd = band_lo(pxcd + 1, j) - lo;
            }
            ty_ = 8 * p8 + j;
            tx_ = lo + rem;
            return;
        }
        const int per_strip = STRIP * tiles_y;
        int sidx = pt_ / per_strip;
        const int nfull = tiles_x / STRIP;
        if (sidx > nfull) sidx = nfull;
        const int wid = sidx < nfull ? STRIP : tiles_x - nfull * STRIP;
        const int q = pt_ - sidx * per_strip;
        ty_ = q / wid;
        tx_ = sidx * STRIP + (q - ty_ * wid);
    };
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float *)lds;
    char *ldsb = reinterpret_cast<char *>(lds);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pt = wave & 3, bt = wave >> 2;
    // ONE lane-linear VGPR lives through the kernel (lane * 16); everything else that depends on the lane is derived from an opaque copy of it where it is
    // used -- hoisted out of the item loop, the ~30 lane-derived values of the epilogue, the transfers and the transform overflow the 256 registers
    // into scratch, and a scratch reload inside a stage waits with vmcnt(0) for every transfer in flight
    const unsigned b_voff = (unsigned)lane * 16u;
    auto lin = [&]() { unsigned v = b_voff; asm volatile("" : "+v"(v)); return v; };
    auto lane_o = [&]() { return (int)(lin() >> 4); };

    const int xcd = blockIdx.x & 7, per = gridDim.x >> 3;
    const int cq = nitems >> 3, cr = nitems & 7;
    int chunk_begin = xcd < cr ? xcd * (cq + 1) : cr * (cq + 1) + (xcd - cr) * cq;
    int chunk_end = chunk_begin + cq + (xcd < cr ? 1 : 0);
    if constexpr (PROG) {   // items = indices into this XCD's own band (tile_coords above)
        int nloc = (tiles_y >> 3) * tiles_x;
        for (int j = 0; j < (tiles_y & 7); j++) nloc += band_lo(xcd + 1, j) - band_lo(xcd, j);
        chunk_begin = 0;
        chunk_end = nloc * NOB;
    }
#ifndef W4_PAIR
#define W4_PAIR 0   // (experiment, profiles/r6_sweeps.log 3) 1: a workgroup runs BOTH 64-plane items of a tile back to back instead of the two items side by side on two workgroups
#endif
    int item0 = chunk_begin + (blockIdx.x >> 3);
    int nmy = (chunk_end - item0 + per - 1) / per;
    if constexpr (W4_PAIR && NOB == 2 && !PROG) {
        const int ntile = nitems >> 1, tq = ntile >> 3, tr = ntile & 7;
        const int tb = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq, te = tb + tq + (xcd < tr ? 1 : 0);
        item0 = tb + (blockIdx.x >> 3);            // (a TILE index in this form)
        if (item0 >= te) return;
        nmy = 2 * ((te - item0 + per - 1) / per);
    } else if (item0 >= chunk_end) return;
    auto item_of = [&](int n) {
        const int nn = n < nmy ? n : nmy - 1;
        if constexpr (W4_PAIR && NOB == 2 && !PROG) return 2 * (item0 + (nn >> 1) * per) + (nn & 1);
        else return item0 + nn * per;
    };

    for (int c = threadIdx.x; c < COUT; c += 512) lds[BIAS_BASE / 4 + c] = d.bias[c];   // (visible after the prologue barrier)
    if constexpr (PROG) {
        if (threadIdx.x < 4) lds[TRIG_BASE / 4 + threadIdx.x] = 0.0f;   // no job to run, no ticket in hand
    }

    // ---- raw tile transfers: chunk ci = piece * 64 + lane -> (channel kk, row R, quad q); wave w < DW sends pieces w, w + DW, ... ----
    const long long cs4 = d.in_cs * 4, rs4 = d.in_rs * 4;     // bytes
    constexpr int DW = W4_DMA4 ? 4 : 8;                        // waves that issue transfers
    constexpr int RJ = (RAW_PIECES + DW - 1) / DW;             // raw pieces per such wave (the last one: waves < RAW_PIECES - (RJ - 1) * DW = 3 only)
    constexpr int UQ = 36 / DW + (36 % DW ? 1 : 0);            // U pieces per such wave (8 waves: the fifth from waves < 4 only)
    unsigned voff[RJ];
    const char *a_base;
    int xlim_r;                                                // in_w - x0 of the tile the raw cursor is in (patch columns >= it are outside the plane)
    auto tile_offsets = [&](int it) {
        int ty_, tx_;
        tile_coords(it / NOB, ty_, tx_);
        const int lane_t = lane_o();   // (nothing of this hoisted out of the item loop)
        const int y0 = ty_ * ROWS - d.wino_py + d.off_y, x0 = tx_ * 32 + d.off_x;
        const int yb = clampi(y0, 0, d.in_h - 1);
        a_base = reinterpret_cast<const char *>(d.in) + (long long)yb * rs4;
        W4B_ONLY(a_base += (long long)(it / bd.items) * bd.in_bs * 4;)   // (batch: the image's planes, on the scalar base only)
        xlim_r = d.in_w - x0;
        if constexpr (IN_NHWC) {
            // NHWC input (32 planes: a pixel = one 128-byte line, written by conv3x3_first / conv3x3_wino): a chunk = channels 4 s .. 4 s + 3 of ONE pixel,
            // chunk index R * 36 + (x % 4) * 9 + x / 4 -- the pixels of a row grouped by column mod 4, so that the eight block columns of a patch
            // position are consecutive chunks (conflict-free ds_read_b32 of a lane's channel); columns clamped (replicate) like the rows
            xlim_r = 64;   // (nothing to mask)
#pragma unroll
            for (int jj = 0; jj < RJ; jj++) {
                int ci = (jj * DW + wave) * 64 + lane_t;
                ci = ci < (ROWS + 2) * 36 ? ci : (ROWS + 2) * 36 - 1;
                const int R = ci / 36, slot = ci - R * 36;
                const int x = 4 * (slot % 9) + slot / 9;
                const int gy = clampi(y0 + R, 0, d.in_h - 1) - yb;
                const int gx = clampi(x0 + x, 0, d.in_w - 1);
                voff[jj] = (unsigned)((long long)gy * rs4 + (long long)gx * (CIN * 4));
            }
            return;
        }
        const int xq_last = (d.in_w - 1) & ~3;
#pragma unroll
        for (int jj = 0; jj < RJ; jj++) {
            const int ci = (jj * DW + wave) * 64 + lane_t;
            int kk = ci / CHS;
            kk = kk < 4 ? kk : 3;
            const int rem = ci - kk * CHS;
            int R = rem / 9;
            const int q = rem - R * 9;
            R = R < ROWS + 2 ? R : ROWS + 1;
            const int gy = clampi(y0 + R, 0, d.in_h - 1) - yb;
            int gx = x0 + 4 * q;
            gx = gx < xq_last ? gx : xq_last;
            voff[jj] = (unsigned)((long long)kk * cs4 + (long long)gy * rs4 + (long long)gx * 4);
        }
    };
    // LDS destinations of the transfers are (wave base + immediate): as precomputed wave-uniform values the ~50 of them are hoisted out of the loops
    // and the SGPR file overflows into VGPR lanes and scratch
    const unsigned wbase = (unsigned)__builtin_amdgcn_readfirstlane(lds0 + (unsigned)wave * 1024u);
    // raw piece jj * 8 + wave of 4-channel slice `slice` of the tile a_base / voff describe, into the raw buffer at byte offset roff
    auto dma_raw = [&](auto JJ, unsigned roff, int slice) {
        constexpr int jj = decltype(JJ)::value;
        const char *sbase = a_base + (long long)slice * (IN_NHWC ? 16 : 4 * cs4);
        lds_dma16_si<jj * DW * 1024u>(sbase, voff[jj], wbase + roff);
    };
    // U of (64-plane block ob, stage s_): 36 pieces of 1 KiB (one per xi); wave w < DW sends xi = w, w + DW, ...
    const char *wpk_w = reinterpret_cast<const char *>(d.wpk) + (size_t)wave * 1024;
    auto dma_u = [&](int ob, int s_, auto SLOT, auto Q) {     // piece xi = DW q + wave
        constexpr unsigned slot = decltype(SLOT)::value;
        constexpr int q = decltype(Q)::value;
        const char *sbase = wpk_w + ((size_t)(ob * NST + s_) * 36 + q * DW) * 1024;
        lds_dma16_si<U_BASE + slot * U_BYTES + q * DW * 1024u>(sbase, b_voff, wbase);
    };
#ifndef W4_DMA_BASES
#define W4_DMA_BASES 1   // 1: a stage's U pieces go off scalar bases formed ONCE per stage / per pair of pieces (immediate offsets -4096 | 0), 0: every piece forms its own
#endif
    // (one instantiation -- 32 planar planes in, 128 NHWC planes out, not on the default path -- spills four registers with the two more live scalars: it keeps the old form)
    constexpr bool DMAB = W4_DMA_BASES && W4_DMA4 && !(CIN == 32 && COUT == 128 && !OUT_PLANAR && !IN_NHWC && !FUSE7);
    // the same off a base the caller keeps: u_pair = (this wave's piece q | 1 of the stage), pieces q even at -4096, q odd at 0
    auto dma_u_pair = [&](const char *u_pair, auto SLOT, auto Q) {
        constexpr unsigned slot = decltype(SLOT)::value;
        constexpr int q = decltype(Q)::value;
        lds_dma16_sio<U_BASE + slot * U_BYTES + q * DW * 1024u, (q & 1) ? 0 : -(DW * 1024)>(u_pair, b_voff, wbase);
    };

    // ---- addressing ----
    // MFMA operands: lane-linear 16-byte quads, (wave-uniform base) + lane * 16: A = U at U_BASE + slot * U_BYTES + pt * 1024 + (xi / 4) * 4096,
    // B = V at V_BASE + slot * V_BYTES + bt * 1024 + (xi / 4) * 2048.  ONE lane-linear VGPR (b_voff) + SGPR bases: the copies the compiler would
    // otherwise keep per base cost registers this kernel does not have.
    const unsigned ua_u = U_BASE + (unsigned)pt * 1024u, va_u = V_BASE + (unsigned)bt * 1024u;
#ifndef W4_KEEP_BASES
#define W4_KEEP_BASES 1   // 1: the operand base addresses (U slot 0 / 1, V) live in three registers of their own; 0: rebuilt from the lane register where used
#endif
    // The operand bases of a stage: with W4_KEEP_BASES they are three more lane-linear registers that live through the kernel (a ds_read's 16-bit immediate
    // reaches both V slots from one base, U's two slots need one each); rebuilt per use they were 7 VALU instructions per wave and stage -- and a VALU
    // instruction is 4 cycles of a SIMD that issues nothing else meanwhile (DESIGN.md 3)
    // (formed at the head of a phase's copy of the item loop and again behind every epilogue -- lane_regs() below --, so that they do not live through the
    // epilogue: with b_voff, which they are formed from, that is room for five of the transform values in flight there)
    unsigned ua0_v = 0, ua1_v = 0, va_v = 0;
    auto ua_of = [&](unsigned slot) { return W4_KEEP_BASES ? ldsb + (slot ? ua1_v : ua0_v) : ldsb + (lin() + (ua_u + slot * U_BYTES)); };
    auto va_of = [&](unsigned slot) { return W4_KEEP_BASES ? ldsb + va_v + slot * V_BYTES : ldsb + (lin() + (va_u + slot * V_BYTES)); };
    // transformer lane (r, kk, c) = block (block row 2 bt + r, column c), channel kk: patch row i, columns 0..3 = chunk (kk, 4 (2 bt + r) + i, c),
    // columns 4, 5 = the first half of chunk (kk, same row, c + 1)
#ifndef W4_KEEP_TR
#define W4_KEEP_TR 1   // 1: the transform's patch-read and V-write lane offsets live in two registers of their own (0: rebuilt from the lane register per quarter)
#endif
    auto tr_rd_calc = [&]() {
        const int l = lane_o(), tr_r = l >> 5, tr_k = (l >> 3) & 3, tr_c = l & 7;
        return IN_NHWC ? (unsigned)((4 * (2 * bt + tr_r) * 36 + tr_c) * 16 + tr_k * 4)                // + buffer + (i * 36 + (j & 3) * 9 + (j >> 2)) * 16
                       : (unsigned)((tr_k * CHS + 4 * (2 * bt + tr_r) * 9 + tr_c) * 16);        // + buffer + i * 144 (+ 16)
    };
    // V-slot address of this lane's patch in the fragment order lane = 16 kk + block (+ slot * V_BYTES + (xi / 4) * 2048)
    auto tr_wr_calc = [&]() {
        const int l = lane_o(), tr_r = l >> 5, tr_k = (l >> 3) & 3, tr_c = l & 7;
        return V_BASE + (unsigned)bt * 1024u + (unsigned)((tr_k * 16 + tr_r * 8 + tr_c) * 16);
    };
    unsigned tr_rd_v = 0, tr_wr_v = 0;
    auto lane_regs = [&]() {   // a dozen VALU instructions
        if constexpr (W4_KEEP_BASES) {
            ua0_v = lin() + ua_u; ua1_v = lin() + (ua_u + U_BYTES); va_v = lin() + va_u;
            asm volatile("" : "+v"(ua0_v), "+v"(ua1_v), "+v"(va_v));
        }
        if constexpr (W4_KEEP_TR) {
            tr_rd_v = tr_rd_calc(); tr_wr_v = tr_wr_calc();
            asm volatile("" : "+v"(tr_rd_v), "+v"(tr_wr_v));
        }
    };
    auto tr_rd = [&]() { return W4_KEEP_TR ? tr_rd_v : tr_rd_calc(); };
    auto tr_wr = [&]() { return W4_KEEP_TR ? tr_wr_v : tr_wr_calc(); };

    // The input transform V = B^T d B of a patch set (16 blocks x 4 channels = one patch per lane) by ONE wave in FOUR QUARTERS over four consecutive
    // stages, the 36 values in REGISTERS in between:
    //   Q0 (stage n - 4)  the raw patch (6 x (ds_read_b128 + ds_read_b64)), columns outside the plane zeroed, the row pass d B of rows 0..2 (3 x 14 fma / add)
    //   Q1 (stage n - 3)  the row pass of rows 3..5
    //   Q2 (stage n - 2)  the column pass B^T (.) of columns 0..2
    //   Q3 (stage n - 1)  the column pass of columns 3..5, V of stage n as nine ds_write_b128 into the slot stage n - 2 has read
    // With PH = (pt - 2 bt) mod 4 a wave runs quarter (stage - PH) mod 4: it transforms the slices n = PH (mod 4) of its block tile, every wave carries
    // the same 42 VALU instructions in every stage, and the two waves of a SIMD (same pt) are two quarters apart (raw reads beside pure arithmetic).
    // The pipeline runs ACROSS items (the last four stages of an item work on the first slices of the next): the three waves of a block tile that
    // are in mid-transform at an item's end keep their 36 values in registers across the epilogue (pin_dd below; PARK: in the U slot and the 18 KiB that
    // are idle then).  Nothing else of a transform touches LDS between its raw reads and its V writes: round 4's
    // earlier forms parked the intermediates of EVERY transform in the V ring (row-pass waves -> column-pass waves), and that traffic alone cost 0.7
    // of layer 6's 6.7 ms (timing-only ablation, profiles/r4_sweeps.log 8).
    // ---- PROG: arrivals and gather jobs (see the comment above the kernel) ----
    const int ngroups = (tiles_x + GW - 1) / GW;
    // lane l < 4 of an item at tile (r, tx): the job it feeds -- (r - (l & 1), tx / 8 - (l >> 1)); the left neighbour group only from the group's first column
    auto job_of_lane = [&](int item, int l, int &jr, int &jg) {
        int r, tx;
        tile_coords(item / NOB, r, tx);
        jr = r - (l & 1);
        jg = tx / GW - (l >> 1);
        return l < 4 && jr >= 0 && ((l >> 1) == 0 || ((tx & (GW - 1)) == 0 && tx > 0));
    };
    auto job_target = [&](int jr, int jg) {   // arrivals that complete job (jr, jg)
        const int rows = jr + 1 < tiles_y ? 2 : 1;
        const int c1 = (jg + 1) * GW + 1;
        return NOB * rows * ((c1 < tiles_x ? c1 : tiles_x) - jg * GW);
    };
    // The counter buffer (zeroed by the launcher in front of every launch): [0, njobs) arrivals per job | [njobs, 2 njobs) the READY QUEUE, slot -> job + 1 |
    // head, tail.  The workgroup whose arrival completes a job only PUSHES it (tail++, then the slot); any workgroup that sees head < tail at an item
    // boundary draws a ticket (head++) and runs the job of that slot at its next boundary.  (Letting the last arriver run the job itself fed back on
    // itself: the slowest workgroup of a neighbourhood is the last arriver every round, got all its jobs -- +20 % on the launch, measured.)
    // All of it is done by wave 7, which issues neither tap-plane stores nor transfers: the compiler's wait for a returned value is vmcnt(0), and in a
    // storing wave that waits for the stores just issued as well.
    const int njobs = tiles_y * ngroups;
    unsigned *const q_slots = d.prog_cnt + njobs, *const q_head = d.prog_cnt + 2 * njobs, *const q_tail = q_head + 1;
    unsigned *const lds_action = reinterpret_cast<unsigned *>(ldsb + TRIG_BASE), *const lds_ticket = lds_action + 1;   // job + 1 to run now | slot + 1 drawn, not yet run
    constexpr int CW = 7;   // the control wave
    // control wave, early in the epilogue: count the arrival of `item` (whose tap planes have drained) on its jobs -- every lane keeps what its job's
    // counter held before --, and look at the queue: the slot of the ticket in hand, or head and tail
    auto prog_early = [&](int item, unsigned &tick, unsigned &q0, unsigned &q1) {
        tick = 0xFFFFFFFFu;
        if (item >= 0) {
            int jr, jg;
            if (job_of_lane(item, lane_o(), jr, jg)) tick = __hip_atomic_fetch_add(d.prog_cnt + (jr * ngroups + jg), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const unsigned t = *lds_ticket;
        q0 = __hip_atomic_load(t ? q_slots + (t - 1) : q_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        q1 = __hip_atomic_load(q_tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // control wave, late in the epilogue: push the jobs the arrivals completed; take the job of the ticket in hand if its slot has been filled, or draw a
    // ticket if a ready job has none -> the LDS words every wave reads behind the next barrier
    auto prog_late = [&](int item, unsigned tick, unsigned q0, unsigned q1) {
        if (item >= 0) {
            int jr, jg;
            const bool valid = job_of_lane(item, lane_o(), jr, jg);
            if (valid && tick == (unsigned)(job_target(jr, jg) - 1)) {   // this arrival was the job's last one
                const unsigned slot = __hip_atomic_fetch_add(q_tail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(q_slots + slot, (unsigned)(jr * ngroups + jg) + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        unsigned t = *lds_ticket, action = 0;
        if (t) {
            if (q0) { action = q0; t = 0; }
        } else if ((int)(q1 - q0) > 0) {
            unsigned h = 0;
            if (lane_o() == 0) h = __hip_atomic_fetch_add(q_head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            h = (unsigned)__builtin_amdgcn_readfirstlane((int)h);
            t = h < (unsigned)njobs ? h + 1 : 0;   // (a ticket past the last job: every job has been drawn)
        }
        if (lane_o() == 0) { *lds_action = action; *lds_ticket = t; }
    };
    // every wave: run the job the control wave has named
    auto prog_run = [&]() {
        const unsigned action = (unsigned)__builtin_amdgcn_readfirstlane((int)*lds_action);
        if (action) {
            W4ProgJob a;
            a.G = d.out; a.ts = d.out_ts; a.gs = d.out_gs; a.rs = d.out_rs;
            a.out = d.g_out; a.out_rs = d.g_out_rs; a.bias = d.g_bias; a.flags = d.prog_flags; a.epoch = d.prog_epoch;
            a.g_h = d.g_h; a.g_w = d.g_w; a.g_off = d.g_off; a.wino_py = d.wino_py; a.ngroups = ngroups;
            w4_prog_job<NOB>(a, (int)(action - 1) / ngroups, (int)(action - 1) % ngroups);
        }
        return action;
    };

    float dd[36];
    auto raw_read = [&](const char *src, auto I_) {          // patch row i
        constexpr int i = decltype(I_)::value;
        if constexpr ((W4_ABL & 2) != 0) {
            static_for<0, 6>([&](auto JJ) { dd[i * 6 + decltype(JJ)::value] = (float)(i + decltype(JJ)::value); });
        } else if constexpr (IN_NHWC) {
            static_for<0, 6>([&](auto JJ) {
                constexpr int j = decltype(JJ)::value;
                dd[i * 6 + j] = *reinterpret_cast<const float *>(src + (i * 36 + (j & 3) * 9 + (j >> 2)) * 16);
            });
        } else {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(src + i * 144);
            const f32x2 b = *reinterpret_cast<const f32x2 *>(src + i * 144 + 16);
            dd[i * 6 + 0] = a[0]; dd[i * 6 + 1] = a[1]; dd[i * 6 + 2] = a[2]; dd[i * 6 + 3] = a[3];
            dd[i * 6 + 4] = b[0]; dd[i * 6 + 5] = b[1];
        }
    };
    auto raw_mask = [&](int xlim) {                           // patch columns outside the plane: zero (wave-uniform test first)
        if (xlim < 34) {
            const int lim = xlim - 4 * (lane_o() & 7);
            static_for<0, 36>([&](auto E) {
                constexpr int e = decltype(E)::value;
                dd[e] = (e % 6) < lim ? dd[e] : 0.0f;
            });
        }
    };
    // (the pins keep a pass in the stage it was written in: without them the compiler sinks it into the stage that consumes its results)
    auto row_pass = [&](auto I_) {                            // s[i][.] = d[i][.] B
        constexpr int i = decltype(I_)::value;
        if constexpr (!(W4_ABL & 3)) bt6(dd[i * 6 + 0], dd[i * 6 + 1], dd[i * 6 + 2], dd[i * 6 + 3], dd[i * 6 + 4], dd[i * 6 + 5]);
        if constexpr (!(W4_ABL & 3)) asm volatile("" : "+v"(dd[i * 6 + 0]), "+v"(dd[i * 6 + 1]), "+v"(dd[i * 6 + 2]), "+v"(dd[i * 6 + 3]), "+v"(dd[i * 6 + 4]), "+v"(dd[i * 6 + 5]));
    };
    auto col_pass = [&](auto J_) {                            // V[.][j] = B^T s[.][j]
        constexpr int j = decltype(J_)::value;
        if constexpr (!(W4_ABL & 3)) bt6(dd[0 * 6 + j], dd[1 * 6 + j], dd[2 * 6 + j], dd[3 * 6 + j], dd[4 * 6 + j], dd[5 * 6 + j]);
        if constexpr (!(W4_ABL & 3)) asm volatile("" : "+v"(dd[0 * 6 + j]), "+v"(dd[1 * 6 + j]), "+v"(dd[2 * 6 + j]), "+v"(dd[3 * 6 + j]), "+v"(dd[4 * 6 + j]), "+v"(dd[5 * 6 + j]));
    };
    // quad q of the fragment order = positions xi = 4 q .. 4 q + 3; position (i, j) sits at xi_of(i, j), its value in dd[6 i + j]
    auto v_write = [&](char *dst, auto Q_) {
        constexpr int q = decltype(Q_)::value;
        if constexpr (!(W4_ABL & 2))
        {
#ifdef W4_VW32
            static_for<0, 4>([&](auto E_) { constexpr int e = decltype(E_)::value; *reinterpret_cast<float *>(dst + q * 2048 + e * 4) = dd[w4p_dd_of(4 * q + e)]; });
#else
            *reinterpret_cast<f32x4 *>(dst + q * 2048) = f32x4{dd[w4p_dd_of(4 * q)], dd[w4p_dd_of(4 * q + 1)], dd[w4p_dd_of(4 * q + 2)], dd[w4p_dd_of(4 * q + 3)]};
#endif
        }
    };

    // The 36 values of a transform in flight at an item's end (PH != 0) stay in REGISTERS across the epilogue: its row transform works in place on the
    // accumulators and the operand ring is idle, so the file holds them.  The pins keep them where they are: nothing of a transform is sunk into or
    // hoisted across the epilogue, nothing is rematerialised.  PARK (the PROG forms, whose epilogue calls w4_prog_job -- values alive across a call
    // go through scratch: 7 spills measured for 64 planes out): the values are parked in LDS instead, in U slot 1 and the spare 18 KiB that are idle then --
    // nine ds_write_b128, nine ds_read_b128 and a workgroup barrier of their own per item, as in every form before.
    constexpr bool PARK = PROG;
    auto pin_dd = [&]() {
        float(&v)[36] = dd;   // (an asm operand alone does not capture dd into a nested generic lambda: six rows written out)
        asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]));
        asm volatile("" : "+v"(v[6]), "+v"(v[7]), "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]));
        asm volatile("" : "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15]), "+v"(v[16]), "+v"(v[17]));
        asm volatile("" : "+v"(v[18]), "+v"(v[19]), "+v"(v[20]), "+v"(v[21]), "+v"(v[22]), "+v"(v[23]));
        asm volatile("" : "+v"(v[24]), "+v"(v[25]), "+v"(v[26]), "+v"(v[27]), "+v"(v[28]), "+v"(v[29]));
        asm volatile("" : "+v"(v[30]), "+v"(v[31]), "+v"(v[32]), "+v"(v[33]), "+v"(v[34]), "+v"(v[35]));
    };

    // A run-time "which quarter now" around the stage bodies joins 144 accumulators in phi nodes and the register allocator gives up: the item loop exists
    // four times (one copy per PH, unrolled by four stages with the quarters fixed at compile time) and a wave picks its copy once.
    auto run = [&](auto PH_) {
    constexpr int PH = decltype(PH_)::value;
    using C0 = std::integral_constant<int, 0>;
    using C1 = std::integral_constant<int, 1>;
    using U0 = std::integral_constant<unsigned, 0u>;
    lane_regs();
    // PARK: where this wave parks across an epilogue: six parkers (three per block tile) x 9 KiB = U slot 1 (idle behind the last stage's closing barrier) + the spare 18 KiB
    const unsigned park_u = (bt * 3 + PH - 1) < 4 ? U_BASE + U_BYTES + (unsigned)(bt * 3 + PH - 1) * 9216u : SPARE_BASE + (unsigned)(bt * 3 + PH - 1 - 4) * 9216u;
    auto park = [&]() {
        char *pa = ldsb + (lin() + park_u);
        static_for<0, 9>([&](auto Q_) {
            constexpr int q = decltype(Q_)::value;
            *reinterpret_cast<f32x4 *>(pa + q * 1024) = f32x4{dd[4 * q], dd[4 * q + 1], dd[4 * q + 2], dd[4 * q + 3]};
        });
    };
    auto unpark = [&]() {
        const char *pa = ldsb + (lin() + park_u);
        static_for<0, 9>([&](auto Q_) {
            constexpr int q = decltype(Q_)::value;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(pa + q * 1024);
            dd[4 * q] = v[0]; dd[4 * q + 1] = v[1]; dd[4 * q + 2] = v[2]; dd[4 * q + 3] = v[3];
        });
    };
    // a whole quarter outside the stages (kernel prologue)
    auto quarter = [&](auto Q_, const char *src, char *dst, int xlim) {
        constexpr int q = decltype(Q_)::value;
        if constexpr (q == 0) {
            static_for<0, 6>([&](auto I) { raw_read(src, I); });
            raw_mask(xlim);
        }
        if constexpr (q < 2) static_for<3 * q, 3 * q + 3>([&](auto I) { row_pass(I); });
        else static_for<3 * (q - 2), 3 * (q - 2) + 3>([&](auto J) { col_pass(J); });
        if constexpr (q == 3) static_for<0, 9>([&](auto Q) { v_write(dst, Q); });
    };
    // ---- kernel prologue: raw slices 0..2 and U(stage 0) of the first item; the quarters that precede stage 0 (slice 0 whole -> V slot 0, slice 1 Q0..Q2,
    //      slice 2 Q0 Q1); raw slices 3..5; slice 3 Q0 ----
    tile_offsets(item_of(0));
    int xlim_cur = xlim_r;                                      // in_w - x0 of the current item's tile
    auto raw_all = [&](unsigned roff, int slice) {              // this wave's pieces of a slice
        if (wave < DW) {
            static_for<0, RJ - 1>([&](auto JJ) { dma_raw(JJ, roff, slice); });
            if (wave < RAW_PIECES - (RJ - 1) * DW) dma_raw(std::integral_constant<int, RJ - 1>{}, roff, slice);
        }
    };
    for (int sl = 0; sl < 3; sl++) raw_all((unsigned)sl * RAW_BYTES, sl);
    if (wave < DW) {
        const int ob0 = item_of(0) % NOB;
        static_for<0, UQ - 1>([&](auto Q) { dma_u(ob0, 0, U0{}, Q); });
        if (wave < 36 - (UQ - 1) * DW) dma_u(ob0, 0, U0{}, std::integral_constant<int, UQ - 1>{});
    }
    W2XC_WAIT_VMCNT(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr (PH < 3) {
        const char *src = ldsb + PH * RAW_BYTES + tr_rd();
        static_for<0, 4 - PH>([&](auto Q) { quarter(Q, src, ldsb + tr_wr(), xlim_cur); });
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    for (int sl = 3; sl < 6; sl++) raw_all((unsigned)(sl - 3) * RAW_BYTES, sl);
    W2XC_WAIT_VMCNT(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr (PH == 3) quarter(C0{}, ldsb + tr_rd(), nullptr, xlim_cur);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    // MFMA operand quads (four xi per ds_read_b128 and operand), read W4_PF groups of four MFMAs ahead.  The closing wait and the barrier of a stage sit in
    // front of its LAST group: behind the barrier the wave reads the first group(s) of the NEXT stage and still has four MFMAs of this one to issue
    // while they arrive -- with the barrier behind the last MFMA every stage began with an exposed LDS round trip (~400 of ~3000 cycles, s_memtime).
    constexpr int PF = W4_PF;
    static_assert(PF == 1 || PF == 2, "operand look-ahead");
    f32x4 a4[PF + 1], b4[PF + 1];
    // register buffer of operand group g of a stage of parity par: g mod 3 with two groups of look-ahead; with one, two buffers whose roles swap with the
    // stage's parity (group 8 and the next stage's group 0 are alive together)
    auto load_first = [&](unsigned slot) {
        const char *ua = ua_of(slot);
        const char *va = va_of(slot);
        static_for<0, PF>([&](auto G) {
            constexpr int g = decltype(G)::value;
            const int b = PF == 2 ? g : (int)slot;
            a4[b] = *reinterpret_cast<const f32x4 *>(ua + g * 4096);
            b4[b] = *reinterpret_cast<const f32x4 *>(va + g * 2048);
        });
    };
    unsigned rd = RAW_BYTES, mid = 2 * RAW_BYTES, fr = 0;   // raw buffers of slice s + 4 (Q0 reads it), s + 5, and the one Q0 of the last stage has read (this stage's transfer: s + 6)
    int stamp = 0;
    (void)stamp;
    W4_STAMP(stamp++);
    for (int n = 0; n < nmy; n++) {
        const int item = item_of(n), item_n = item_of(n + 1);
        f32x4 acc[36];   // (first written by the item's first stage: its MFMAs take 0 as their accumulator input -- 144 v_mov per wave and item less)

        // one stage; J = global stage count mod 4 (NST is a multiple of 4: = s mod 4)
        auto stage = [&](auto J_, auto FIRST_, int s) {
            constexpr int J = decltype(J_)::value;
            constexpr bool FIRST = decltype(FIRST_)::value;   // the item's first stage
            constexpr int QT = (J - PH) & 3;                                              // this wave's quarter, of slice s + 4 - QT
            constexpr unsigned par = J & 1, nxt = par ^ 1u;                               // U / V slot of this stage and of the next
            int u_ob = item % NOB, u_s = s + 1;
            if (s == NST - 1) { u_ob = item_n % NOB; u_s = 0; }
            const char *ua = ua_of(par);
            const char *va = va_of(par);
            // this wave's first U piece of the stage it transfers, formed once (left to the compiler every piece recomputed it from (u_ob, u_s): ~6 scalar
            // instructions per piece in front of an MFMA that waits for them in program order)
            const char *u_st = wpk_w + (size_t)(u_ob * NST + u_s) * 36864, *u_pair = u_st;
            if constexpr (DMAB) asm volatile("" : "+s"(u_st));
            const char *srcQ = nullptr;
            char *dstQ = nullptr;
            if constexpr (QT == 0) srcQ = ldsb + (rd + tr_rd());
            if constexpr (QT == 3) dstQ = ldsb + (tr_wr() + nxt * V_BYTES);
            const int xlimQ = s + 4 < NST ? xlim_cur : xlim_r;
            if constexpr (J == 2) {
                if (s == NST - 6) tile_offsets(item_n);   // from this stage on the raw cursor (six slices ahead) is in the next item's tile
            }
            const int r_slice = s + 6 < NST ? s + 6 : s + 6 - NST;
            static_for<0, 36>([&](auto XI) {
                constexpr int xi = decltype(XI)::value;
                constexpr int g = xi >> 2;
                if constexpr (xi == 32) {
                    // ---- the stage's close, in front of its last four MFMAs ----
                    W4_STAMP(stamp++);
                    // U of the next stage and the raw slice issued one stage ago (Q0 of the NEXT stage reads it) have landed; this stage's raw pieces --
                    // the youngest transfers -- may still fly
                    if constexpr ((W4_ABL & 32) != 0) W2XC_WAIT_VMCNT(0);
                    else if (wave < RAW_PIECES - (RJ - 1) * DW) wait_vmcnt_n(RJ);
                    else if (wave < DW) wait_vmcnt_n(RJ - 1);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    W4_STAMP(stamp++);
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                    { const unsigned tr = rd; rd = mid; mid = fr; fr = tr; }
                    if (s != NST - 1) {                     // (an item's last stage: the epilogue comes first, the item loop reads them)
                        if constexpr (PF == 2) load_first(nxt);
                        else {
                            a4[nxt] = *reinterpret_cast<const f32x4 *>(ua_of(nxt));
                            b4[nxt] = *reinterpret_cast<const f32x4 *>(va_of(nxt));
                        }
                    }
                    W4_STAMP(stamp++);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr ((xi & 3) == 0 && g + PF < 9 && !(W4_ABL & 128)) {
                    constexpr int b = PF == 2 ? (g + PF) % 3 : ((g + 1 + (int)par) & 1);
                    a4[b] = *reinterpret_cast<const f32x4 *>(ua + (g + PF) * 4096);
                    b4[b] = *reinterpret_cast<const f32x4 *>(va + (g + PF) * 2048);
                    __builtin_amdgcn_sched_barrier(0);
                }
                {
                    constexpr int b = PF == 2 ? g % 3 : ((g + (int)par) & 1);
                    // (as an instruction with the accumulator tied: left to the register allocator, most of these MFMAs get a destination other than
                    // their accumulator input, the 144 accumulators migrate through the file and some are spilled inside the stages)
                    if constexpr (FIRST) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, 0" : "=v"(acc[xi]) : "v"(a4[b][xi & 3]), "v"(b4[b][xi & 3]));
                    else asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[xi]) : "v"(a4[b][xi & 3]), "v"(b4[b][xi & 3]));
                }
                __builtin_amdgcn_sched_barrier(0);
                // the stage's other work, behind the first MFMA slots: transfers (U pieces first, the raw pieces last: the closing wait leaves them in
                // flight), then this wave's quarter of the input transform
                constexpr int TSTEP = W4_DMA4 ? 1 : 2, tk = xi >= 1 && (xi - 1) % TSTEP == 0 ? (xi - 1) / TSTEP : -1;   // transfer slot behind MFMA xi
                if constexpr (tk >= 0 && tk < UQ && !(W4_ABL & 16)) {
                    constexpr int q = tk;
                    if constexpr (DMAB) {
                        if (wave < (q == UQ - 1 ? 36 - (UQ - 1) * DW : DW)) {
                            if constexpr ((q & 1) == 0) {   // the base of pieces q and q + 1: one 64-bit scalar addition per pair
                                u_pair = u_st + (q + 1) * (DW * 1024);
                                asm volatile("" : "+s"(u_pair));
                            }
                            dma_u_pair(u_pair, std::integral_constant<unsigned, nxt>{}, std::integral_constant<int, q>{});
                        }
                    } else {
                        if (wave < (q == UQ - 1 ? 36 - (UQ - 1) * DW : DW)) dma_u(u_ob, u_s, std::integral_constant<unsigned, nxt>{}, std::integral_constant<int, q>{});
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (tk >= UQ && tk < UQ + RJ && !(W4_ABL & 32)) {
                    constexpr int jj = tk - UQ;      // slice s + 6 into the buffer Q0 of stage s - 1 has read
                    // (the slice base of these two or three pieces formed once per stage as well: two more live scalars, 4 VGPR spills in the planar kernel, slower)
                    if (wave < (jj == RJ - 1 ? RAW_PIECES - (RJ - 1) * DW : DW)) dma_raw(std::integral_constant<int, jj>{}, fr, r_slice);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (QT == 0 && xi < 2) {
                    raw_read(srcQ, std::integral_constant<int, 3 * xi>{});
                    raw_read(srcQ, std::integral_constant<int, 3 * xi + 1>{});
                    raw_read(srcQ, std::integral_constant<int, 3 * xi + 2>{});
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (xi >= W4P_T0 && xi < W4P_T0 + 3) {
                    if constexpr (QT == 0 && xi == W4P_T0) raw_mask(xlimQ);
                    if constexpr (QT < 2) row_pass(std::integral_constant<int, 3 * QT + xi - W4P_T0>{});
                    else col_pass(std::integral_constant<int, 3 * (QT - 2) + xi - W4P_T0>{});
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (QT == 3 && xi >= W4P_T0 + 3 && xi < W4P_T0 + 6) {
                    v_write(dstQ, std::integral_constant<int, 3 * (xi - (W4P_T0 + 3))>{});
                    v_write(dstQ, std::integral_constant<int, 3 * (xi - (W4P_T0 + 3)) + 1>{});
                    v_write(dstQ, std::integral_constant<int, 3 * (xi - (W4P_T0 + 3)) + 2>{});
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
        };
        load_first(0u);
        // the loop, rotated by one stage: the first stage of the item is its own copy of the stage body (five copies instead of four)
        stage(std::integral_constant<int, 0>{}, std::true_type{}, 0);
#pragma unroll 1
        for (int s = 1; s < NST; s += 4) {
            stage(std::integral_constant<int, 1>{}, std::false_type{}, s);
            stage(std::integral_constant<int, 2>{}, std::false_type{}, s + 1);
            stage(std::integral_constant<int, 3>{}, std::false_type{}, s + 2);
            if (s + 3 < NST) stage(std::integral_constant<int, 0>{}, std::false_type{}, s + 3);
        }
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // (the last MFMAs' results: the hazard the compiler does not see through the asm)
        xlim_cur = xlim_r;   // (the raw cursor entered the next item's tile five stages ago)
        if constexpr (PH != 0) {   // (PH = 0 has just written the V of the next item's first stage)
            if constexpr (PARK) park();
            else pin_dd();
        }
        {
            // ---- epilogue: Y = A^T M A, bias, LeakyReLU, stores.  C/D of the 16x16 MFMA: lane & 15 = block, register e = plane
            //      4 (lane >> 4) + e of the plane tile ----
            __builtin_amdgcn_s_setprio(2);
            const int ob = item % NOB;
            const int lane_e = lane_o(), t = lane_e & 15, k = lane_e >> 4;
            int tile_y, tile_x;
            tile_coords(item / NOB, tile_y, tile_x);
            const int ty0 = tile_y * ROWS - d.wino_py;
            const int oy = ty0 + 4 * (2 * bt + (t >> 3)), ox = tile_x * 32 + 4 * (t & 7);
            const int plane0 = ob * 64 + pt * 16 + 4 * k;
            float *obase = OUT_PLANAR ? W4B_OUT + (long long)plane0 * d.out_cs + (long long)oy * d.out_rs + ox
                                      : W4B_OUT + (long long)oy * d.out_rs + (long long)ox * COUT + plane0;
            const bool interior = ty0 >= 0 && ty0 + ROWS <= d.out_h && tile_x * 32 + 32 <= d.out_w;   // wave-uniform
            const f32x4 bq = *reinterpret_cast<const f32x4 *>(ldsb + BIAS_BASE + plane0 * 4);
            // FUSE7: the one-plane LAST layer (convertRoutine.cpp:66-76's next iteration) inside this epilogue, "taps as rows": per pixel the nine partial
            // sums T_tap = sum over this wave's 16 planes of w7[plane][tap] * a6[plane] on the MFMA (A = w7 of the planes 4 k + e as 16 x 4, tap = row;
            // B = the activations just computed, lane (k, block) = plane 4 k + e of a pixel of that block), summed over the four plane-tile waves
            // through LDS that is idle between two items, and written as 9 tap planes per 64-plane block: 72 bytes per pixel leave the chip
            // instead of 512, and conv3x3_last_gather adds taps and blocks (0.1 ms instead of the 0.8 ms of conv3x3_last).
            float a7[4];
            if constexpr (FUSE7) {
                const float *w7 = reinterpret_cast<const float *>(d.w7pk) + (size_t)(ob * 4 + pt) * 256 + lane_e;   // [16-plane group][e][lane]
#pragma unroll
                for (int e = 0; e < 4; e++) a7[e] = w7[e * 64];
            }
            // The tap exchange.  PARK (U slot 1 and the spare hold the parked transforms): one ROW STEP at a time through V slot 1 -- [pt][tap][128 pixels]
            // floats, 18 KiB, two workgroup barriers per row step.  Otherwise the whole ITEM at once: behind the last stage's closing barrier U slot 1, V slot 1
            // and the spare 18 KiB are all idle until the next item's first stage fills them, 72 KiB = [pt][tap][512 pixels] floats -- plane tiles 0 and 1 in U
            // slot 1, 2 and 3 in V slot 1 and the spare behind it (V slot 0 and U slot 0, between them, hold the next item's first stage) --, pixel index =
            // row step * 128 + the row step's: two barriers per item.
            constexpr bool SLAB_ITEM = FUSE7 && !PARK;
            constexpr int SLAB_PX = SLAB_ITEM ? 512 : 128;
            char *red = ldsb + V_BASE + V_BYTES;   // (V slot 1: idle until the next item's first stage writes V of its second)
            auto slab_of = [&](int q) {            // plane tile q's [tap][SLAB_PX] floats
                if constexpr (SLAB_ITEM) return ldsb + (q < 2 ? U_BASE + U_BYTES + (unsigned)q * V_BYTES : V_BASE + V_BYTES + (unsigned)(q - 2) * V_BYTES);
                else return red + q * (9 * 128 * 4);
            };
            static_assert(SPARE_BASE == V_BASE + 2 * V_BYTES && U_BYTES == 2 * V_BYTES && V_BYTES == 9 * 512 * 4, "the item's slab");
            // quad `job` of a slab's [tap][pixel quad]s (tap = job / (SLAB_PX / 4)): the four plane tiles summed in the order 0..3, stored into its tap plane
            auto tap_reduce = [&](int job, int tap, int gy, int gx) {
                f32x4 sum = *reinterpret_cast<const f32x4 *>(slab_of(0) + job * 16);
#pragma unroll
                for (int q = 1; q < 4; q++) sum += *reinterpret_cast<const f32x4 *>(slab_of(q) + job * 16);   // (fixed order: reproducible)
                if (gy >= 0 && gy < d.out_h && gx < d.out_w) {
                    float *g = W4B_OUT + (long long)ob * d.out_ts + (long long)tap * d.out_gs + (long long)gy * d.out_rs + gx;
                    if constexpr (PROG) {   // written through: read by the gather job of whichever workgroup arrives last
                        if (gx + 3 < d.out_w) store16_sc1(g, sum);
                        else {
#pragma unroll
                            for (int e = 0; e < 3; e++)
                                if (gx + e < d.out_w) store4_sc1(g + e, sum[e]);
                        }
                    } else if (gx + 3 < d.out_w) *reinterpret_cast<f32x4u *>(g) = sum;   // (dword-aligned: rows of out_w floats)
                    else {
#pragma unroll
                        for (int e = 0; e < 3; e++)
                            if (gx + e < d.out_w) g[e] = sum[e];
                    }
                }
            };
            unsigned tick = 0xFFFFFFFFu, pq0 = 0, pq1 = 0;   // PROG, control wave: what the job counters of the PREVIOUS item's arrivals held; the queue
            (void)tick; (void)pq0; (void)pq1;
            // The row transform A^T M of every column, all four rows at once (10 operations per column and plane; two passes over row PAIRS recompute
            // the four sums and differences: 14): the six accumulators of a (column, plane) are dead behind it, their registers hold its four results.
            float tm[4][6][4];   // [row][column j][plane e]
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    const float m0 = acc[xi_of(0, j)][e], m1 = acc[xi_of(1, j)][e], m2 = acc[xi_of(2, j)][e], m3 = acc[xi_of(3, j)][e],
                                m4 = acc[xi_of(4, j)][e], m5 = acc[xi_of(5, j)][e];
                    const float s1 = m1 + m2, d1 = m1 - m2, s2 = m3 + m4, d2 = m3 - m4;
                    tm[0][j][e] = m0 + s1 + s2;
                    tm[1][j][e] = __builtin_fmaf(1.5f, d2, 0.75f * d1);
                    tm[2][j][e] = __builtin_fmaf(2.25f, s2, 0.5625f * s1);
                    tm[3][j][e] = __builtin_fmaf(3.375f, d2, __builtin_fmaf(0.421875f, d1, m5));
                }
            // PROG: the PREVIOUS item's tap planes (and every transfer but the youngest) have long landed: this wait is all but free here, and makes
            // that item's arrival countable behind the first barrier below
            if constexpr (PROG) W2XC_WAIT_VMCNT(0);
#pragma unroll
            for (int rp = 0; rp < 2; rp++) {
#pragma unroll
                for (int rr = 0; rr < 2; rr++) {
                    const int i = 2 * rp + rr;
                    f32x4 y[4];      // OUT_PLANAR: y[e] = the four pixels of row i of plane e; NHWC: y[j] = the four planes of pixel j
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        float y0, y1, y2, y3;
                        at6(tm[i][0][e], tm[i][1][e], tm[i][2][e], tm[i][3][e], tm[i][4][e], tm[i][5][e], y0, y1, y2, y3);
                        const float w0 = y0 + bq[e], w1 = y1 + bq[e], w2 = y2 + bq[e], w3 = y3 + bq[e];
                        const float l0 = __builtin_amdgcn_fmed3f(w0, 0.1f * w0, 3.402823466e+38f), l1 = __builtin_amdgcn_fmed3f(w1, 0.1f * w1, 3.402823466e+38f);
                        const float l2 = __builtin_amdgcn_fmed3f(w2, 0.1f * w2, 3.402823466e+38f), l3 = __builtin_amdgcn_fmed3f(w3, 0.1f * w3, 3.402823466e+38f);
                        if constexpr (OUT_PLANAR || FUSE7) y[e] = f32x4{l0, l1, l2, l3};
                        else { y[0][e] = l0; y[1][e] = l1; y[2][e] = l2; y[3][e] = l3; }
                    }
                    if constexpr (FUSE7) {
                        // y[e] = the four pixels of row i of plane e (OUT_PLANAR form): D[j] = taps of pixel j of this lane's block over the wave's planes
                        f32x4 D[4];
#pragma unroll
                        for (int j = 0; j < 4; j++) D[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                        for (int e = 0; e < 4; e++)
#pragma unroll
                            for (int j = 0; j < 4; j++) D[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a7[e], y[e][j], D[j], 0, 0, 0);
                        // lane (k, t) holds taps 4 k .. 4 k + 3 of pixel j of block t.  A row step's pixels in the slab [pt][tap][pixel]: p = (block row) * 32 +
                        // (block column) * 4 + j: ONE 16-byte write per tap = the four pixels of this lane's block, eight lanes = 128 contiguous bytes (as
                        // [pt][tap quad][pixel][4] the eight lanes of a write group sat 64 bytes apart: four-way bank conflicts, 9 % of layer 6's LDS cycles)
                        const int p0 = (SLAB_ITEM ? i * 128 : 0) + (2 * bt + (t >> 3)) * 32 + (t & 7) * 4;
                        char *slab = slab_of(pt);
                        if (k < 2) {
#pragma unroll
                            for (int r = 0; r < 4; r++) *reinterpret_cast<f32x4 *>(slab + ((4 * k + r) * SLAB_PX + p0) * 4) = f32x4{D[0][r], D[1][r], D[2][r], D[3][r]};
                        } else if (k == 2) {
                            *reinterpret_cast<f32x4 *>(slab + (8 * SLAB_PX + p0) * 4) = f32x4{D[0][0], D[1][0], D[2][0], D[3][0]};
                        }
                        if constexpr (!SLAB_ITEM) {
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                            __builtin_amdgcn_s_barrier();
                            asm volatile("" ::: "memory");
                            if constexpr (PROG) {
                                // (every wave has drained the previous item's stores in front of this barrier) its arrival, counted by wave 0; the counters'
                                // answers are looked at three row steps further down
                                if (i == 0 && wave == CW) prog_early(n > 0 ? item_of(n - 1) : -1, tick, pq0, pq1);
                                if (i == 3 && wave == CW) prog_late(n > 0 ? item_of(n - 1) : -1, tick, pq0, pq1);
                            }
                            {
                                const int tid = wave * 64 + lane_e;
                                if (tid < 288) {
                                    const int tap = tid >> 5, p = (tid & 31) * 4;     // nine taps x 32 pixel quads
                                    tap_reduce(tid, tap, ty0 + 4 * (p >> 5) + i, tile_x * 32 + (p & 31));
                                }
                            }
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                            __builtin_amdgcn_s_barrier();   // (the slab is rewritten by the next row)
                            asm volatile("" ::: "memory");
                        }
                    } else if constexpr ((W4_ABL & 64) != 0) {
                        if (y[0][0] == 12345.678f) *reinterpret_cast<f32x4 *>(obase) = y[0] + y[1] + y[2] + y[3];
                    } else if constexpr (OUT_PLANAR) {
                        // whole quads: the row stride holds roundup4(out_w) pixels (the launcher checks), columns >= out_w are never read as data
                        if (interior || (oy + i >= 0 && oy + i < d.out_h && ox < d.out_w)) {
#pragma unroll
                            for (int e = 0; e < 4; e++) *reinterpret_cast<f32x4 *>(obase + (long long)e * d.out_cs + (long long)i * d.out_rs) = y[e];
                        }
                    } else if (interior) {
#pragma unroll
                        for (int j = 0; j < 4; j++) *reinterpret_cast<f32x4 *>(obase + (long long)i * d.out_rs + j * COUT) = y[j];
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            if (oy + i >= 0 && oy + i < d.out_h && ox + j < d.out_w) *reinterpret_cast<f32x4 *>(obase + (long long)i * d.out_rs + j * COUT) = y[j];
                    }
                }
            }
            if constexpr (SLAB_ITEM) {
                // the item's taps are in the slab: ONE barrier, then the 9 x 128 pixel quads over all 512 threads (three or fewer each; quad `job` sits at
                // job * 16 of every plane tile's part: lane-linear reads), one barrier before the next item's first stage writes U and V there
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                const int tid = wave * 64 + lane_e;
#pragma unroll
                for (int jb = 0; jb < 3; jb++) {
                    const int job = tid + jb * 512;
                    if (jb < 2 || job < 9 * 128) {
                        const int tap = job >> 7, i = (job >> 5) & 3, p = (job & 31) * 4;     // nine taps x four row steps x 32 pixel quads
                        tap_reduce(job, tap, ty0 + 4 * (p >> 5) + i, tile_x * 32 + (p & 31));
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
            __builtin_amdgcn_s_setprio(0);
            W4_STAMP(stamp++);
            // PROG: the gather jobs the previous item's arrivals completed (the LDS word was written in front of the epilogue's last barrier)
            if constexpr (PROG) prog_run();
        }
        if constexpr (PARK) {
            // the transforms in flight back into registers; the barrier: the next stage's U transfers land on the parking area
            if constexpr (PH != 0) unpark();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        } else {
            // No barrier: the epilogue reads nothing of LDS but the bias (FUSE7: its own last barrier stands between the slab's readers and the next
            // stage's writes), and what the next item's first stage reads and overwrites was settled by the last stage's closing barrier, as between any
            // two stages of an item.
            if constexpr (PH != 0) pin_dd();
            lane_regs();   // (not kept through the epilogue)
        }
    }
    W2XC_WAIT_VMCNT(0);   // drain the speculative transfers before the LDS is released
    if constexpr (PROG) {
        // the workgroup's LAST item: its tap planes have drained (the wait above, every wave), its arrival is counted and what it completed is pushed; then
        // the workgroup works the queue off -- this once with every latency exposed -- until it holds no ticket and sees no ready job without one.  Jobs pushed
        // later are drawn by workgroups still running or by their pusher's own pass through here; a ticket whose slot is still empty is waited for (the slot
        // is filled by a workgroup that is running and waits for nobody).
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        bool first = true;
        for (;;) {
            if (wave == CW) {
                unsigned tick, q0, q1;
                prog_early(first ? item_of(nmy - 1) : -1, tick, q0, q1);
                prog_late(first ? item_of(nmy - 1) : -1, tick, q0, q1);
                unsigned t = *lds_ticket;
                if (*lds_action == 0 && t) {   // a ticket in hand: wait for its slot
                    unsigned q = 0;
                    while ((q = __hip_atomic_load(q_slots + (t - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0) __builtin_amdgcn_s_sleep(8);
                    if (lane_o() == 0) { *lds_action = q; *lds_ticket = 0; }
                }
            }
            const bool was_first = first;
            first = false;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            const unsigned ran = prog_run();
            __builtin_amdgcn_s_barrier();   // (the control wave rewrites the words)
            asm volatile("" ::: "memory");
            // (the first pass looked at the queue BEFORE it pushed what this workgroup's last arrival completed: the pass that ends the loop is one that
            //  has seen the queue after every push of this workgroup -- or the last pusher of the launch would leave with its job still in the queue)
            if (!ran && !was_first) break;
        }
    }
    };
#ifdef W4_ONE_PH   // timing-only (tools/ubench): every wave runs the copy of phase W4_ONE_PH -- wrong results, the same work per stage, a quarter of the hot code
    run(std::integral_constant<int, W4_ONE_PH>{});
    return;
#endif
    switch ((pt - 2 * bt) & 3) {
    case 0: run(std::integral_constant<int, 0>{}); break;
    case 1: run(std::integral_constant<int, 1>{}); break;
    case 2: run(std::integral_constant<int, 2>{}); break;
    default: run(std::integral_constant<int, 3>{}); break;
    }
