// svoxt_tile_reduce.inc -- the second half of a pass of the per-tile backwards, included INSIDE
// grad_fused_kernel (textually: as a function with a dozen pointer parameters the same
// code cost the SH9 instances 70-110 bytes of scratch spills per lane at their 128-register budget, r03).
// In scope: lane, wave, NT, T, R, K, NB, BDS, HALF, NH, KS, C, FMT, COUNT, CHECK (SVOXT_CHK), XF (+ vds, tr); the LDS arrays keys, cnt, order, r_sl,
// r_sg, r_w, r_c, bases, gl, stage, seg, s_nb; grad, gstride, counters; nscan = the records of the pass (slots 0 .. nscan - 1).
// The records of the pass sit in the arrays r_* (table entry = r_sl[.] >> 6 of keys / cnt, ray = r_sl[.] & 63;
// weight, sigma entry and the three coefficients in r_w, r_sg, r_c); wavefront 0 may still be advancing the
// last round.  Exclusive scan of the table's counters (wavefront 1), counting sort of the record numbers by
// feature row, then the reduce: 64 sorted records at a time per wavefront, expanded into their K gradient
// values, summed per feature row and sent out as one atomic row per (tile, pass, row), the K columns in NH
// rounds of 16 (0-15, 16-31, ...: each atomic instruction of a row touches one 64-byte line of a row that starts on
// a 64-byte boundary).
{
    // ---- sort: exclusive scan of the counters -- by wavefront 1, while wavefront 0 still advances
    // the last round (the counters are complete since the round's barrier) -- then the
    // counting sort of the record numbers
    if (wave == 1) {
        const int total = row_table_counts_scan<T>(cnt, lane);
        if (lane == 63) s_nb = total;
    }
    lds_barrier();       // (the phases of a pass hand over through LDS alone: the next round's request and the
                         // gradient atomics stay in flight across their barriers)
    const int nb = __builtin_amdgcn_readfirstlane(s_nb);
    if constexpr (CHECK) {          // the table's counters must add up to the records of the pass
        if (threadIdx.x == 0 && nb != nscan) atomicAdd(counters + kChkBase + 13, 1ull);
    }
    if constexpr (COUNT) {          // distinct feature rows of this pass = occupied table slots
        unsigned long long rows = 0;
        for (int i = threadIdx.x; i < T; i += NT) rows += keys[i] >= 0 ? 1u : 0u;
        rows = wave_sum(rows);
        if (lane == 0 && rows) atomicAdd(counters + 1, rows);
    }
    for (int rr = threadIdx.x; rr < nscan; rr += NT)             // (the records of the pass are slots 0 .. nscan - 1)
        order[SVOXT_CHK(atomicAdd(cnt + SVOXT_CHK((int)(r_sl[SVOXT_CHK(rr, R, 10)] >> 6), T, 8), 1), R, 9)] = (uint16_t)rr;
    lds_barrier();
    // ---- reduce: 64 sorted records at a time per wavefront, the K columns in two rounds
    // (0-15, 16-K: each atomic instruction of a row touches one 64-byte line of a row that
    // starts on a 128-byte boundary)
    for (int base = wave * 64; base < (CHECK ? min(nb, R) : nb); base += NT) {
        const int p = base + lane;
        int my_sl = -1;
        float w = 0.f, sgv = 0.f, cc[3] = {0.f, 0.f, 0.f}, gc[3] = {0.f, 0.f, 0.f};
        // the record's ray's basis values: in registers up to SH9; wider bases are read from LDS column by column
        // (16 / 25 registers across the rounds of columns are more than the kernel's 128 leave)
        constexpr bool BX_REG = NB <= 9;
        float bx[(BX_REG && NB > 0) ? NB : 1];
        int rl = 0;
        if (p < nb) {
            const int rr = SVOXT_CHK((int)order[p], nscan, 10);
            const int v = (int)r_sl[rr];
            my_sl = SVOXT_CHK(v >> 6, T, 11);
            rl = v & 63;
            sgv = r_sg[rr];
#pragma unroll
            for (int c3 = 0; c3 < C; ++c3) cc[c3] = r_c[c3 * R + rr];
            if constexpr (FMT == FMT_SH) {
                w = r_w[rr];
                if constexpr (XF) {             // the record's own basis: its row's matrix applied to its ray's direction
                    const float vd3[3] = {vds[rl * 3], vds[rl * 3 + 1], vds[rl * 3 + 2]};
                    rotated_sh_basis<NB>(tr, SVOXT_CHK(keys[my_sl], tr.M, 12), vd3, bx);
                } else if constexpr (BX_REG) {
#pragma unroll
                    for (int i = 0; i < NB; ++i) bx[i] = bases[rl * BDS + i];
                }
#pragma unroll
                for (int c3 = 0; c3 < C; ++c3) gc[c3] = gl[rl * 3 + c3];
            }
        }
        seg[lane] = my_sl >= 0 ? SVOXT_CHK(keys[my_sl], tr.M, 12) : -1;          // the feature row staged row `lane` belongs to
        const int grp = lane >> 4, sub = lane & 15;
#pragma unroll
        for (int h2 = 0; h2 < NH; ++h2) {
            const int c_lo = h2 * HALF;
            const int ncol = (K - c_lo) < HALF ? (K - c_lo) : HALF;
            if (ncol > 0) {
                if (p < nb) {
                    float* st = stage + lane * KS;
#pragma unroll
                    for (int j = 0; j < HALF; ++j) {
                        const int col = c_lo + j;           // compile-time after unrolling
                        if (col < K) {
                            float val;
                            if (col == K - 1) val = sgv;
                            else if constexpr (FMT == FMT_SH) {
                                const float b = BX_REG ? bx[BX_REG ? col % (NB > 0 ? NB : 1) : 0]
                                                       : bases[rl * BDS + col % (NB > 0 ? NB : 1)];
                                val = w * b * cc[col / (NB > 0 ? NB : 1)] * gc[col / (NB > 0 ? NB : 1)];
                            }
                            else val = cc[col];
                            st[j] = val;
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const bool has = sub < ncol;
                unsigned long long nreq = 0;
                int keyv[16];
                float xv[16];
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    const int row = grp * 16 + t;
                    keyv[t] = seg[row];
                    xv[t] = stage[row * KS + (has ? sub : 0)];
                }
                // the rows are sorted and the empty ones (-1) come last: a run that ends inside the group is a real
                // feature row, only the last run can be the empty one; the row's address in one 32 x 32 -> 64-bit multiply-add
                char* const col_ptr = reinterpret_cast<char*>(grad + c_lo + sub);
                const uint32_t row_bytes = (uint32_t)gstride * 4u;
                int cur = keyv[0];
                float acc = xv[0];
#pragma unroll
                for (int t = 1; t < 16; ++t) {
                    const int key = keyv[t];
                    if (key != cur) {
                        if (has) atomicAdd(reinterpret_cast<float*>(col_ptr + (uint64_t)(uint32_t)cur * row_bytes), acc);
                        if constexpr (COUNT) nreq += sub == 0 ? 1u : 0u;
                        acc = 0.f;
                        cur = key;
                    }
                    acc += xv[t];
                }
                if (cur >= 0 && has) atomicAdd(reinterpret_cast<float*>(col_ptr + (uint64_t)(uint32_t)cur * row_bytes), acc);
                if constexpr (COUNT) {
                    nreq += (cur >= 0 && sub == 0) ? 1u : 0u;
                    nreq = wave_sum(nreq);
                    if (lane == 0 && nreq) atomicAdd(counters, nreq);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
}
