// mf_ivf_scan.inc -- the scan kernel of mf_ivf.hip, included once per form with
//   MF_SCAN_KERNEL   the kernel's name: ivf_scan_kernel (mf_ivf_scan), ivf_scan_allow_kernel (mf_ivf_scan_allow)
//   MF_SCAN_ALLOW    false / true: a row enters a list only where the bit of its cell-ordered position is set in the query's
//                    mask (mf_cells.h), and a block whose word is 0 is not read at all
// Everything else is the same lines for both.  (Text, not a template flag or a shared __device__ body: the unfiltered kernel
// keeps its name and, instruction for instruction, the code it had as the only form -- as an inlined body its schedule moved.)
template <int D>
__global__ __launch_bounds__(64 * MF_CELLS_NW) void MF_SCAN_KERNEL(IvfParams p) {
    constexpr bool ALLOW = MF_SCAN_ALLOW;
    constexpr int CPR = D / 4;
    constexpr int HALF = CPR > 32 ? 32 : CPR;                  // chunks held in registers at once
    __shared__ unsigned long long buf[MF_CELLS_NW][64 + IVF_PEND];  // per wave: its best keys so far [0, 64), then the waiting ones
    __shared__ unsigned long long win[MF_CELLS_NW][64], sorted[MF_CELLS_NW][64];
    __shared__ unsigned long long all[MF_CELLS_NW * 64];
    const int lane = mf_lane(), wave = mf_wave_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    // blockIdx.x = (q * nprobe + probe) * S + slice: everything here is workgroup-uniform (mf_pq.hip has the same lines: mf_cells.h)
    const int64_t wg = blockIdx.x;
    const int slice = (int)(wg % p.S);
    const int probe = (int)((wg / p.S) % p.nprobe);
    const int64_t q = wg / ((int64_t)p.S * p.nprobe);
    const int64_t cell = p.probes[q * p.nprobe + probe];
    int64_t b0 = 0, b1 = 0;
    if (cell >= 0 && cell < p.C) {
        const int64_t c0 = p.cell_blk[cell], nb = p.cell_blk[cell + 1] - c0;
        b0 = c0 + nb * slice / p.S;
        b1 = c0 + nb * (slice + 1) / p.S;
    }
    mf_const_f32 qc = (mf_const_f32)p.q + (size_t)q * D;
    int64_t e0 = 0, e1 = 0;
    if (p.excl_off) {
        e0 = p.excl_off[q];
        e1 = p.excl_off[q + 1];
    }
    // the word of the wave's next block is asked for a block ahead: its load is in flight while this block is scored, so the
    // rows of an admitted block are not kept waiting for it
    const unsigned long long* mask = nullptr;
    unsigned long long next_word = 0ull;
    if constexpr (ALLOW) {
        mask = mf_cells_allow_mask(p.allow, q);
        if (b0 + wave < b1) next_word = mf_cells_allow_word(mask, b0 + wave);
    }
    unsigned long long* mine = buf[wave];
#pragma unroll
    for (int j = 0; j < (64 + IVF_PEND) / 64; ++j) mine[lane + 64 * j] = 0ull;
    unsigned long long tau = 0ull;             // the wave's k-th best key once it holds k: only a larger key matters
    int pend = 0;
    // the k best of the wave's list and what waits behind it, in descending order at the front; the rest cleared
    auto settle = [&]() {
        mf_row_topk_sync<true>();
        const int m = mf_row_topk<(64 + IVF_PEND) / 64, true>(mine, 64 + IVF_PEND, p.k, win[wave], sorted[wave]);
        const unsigned long long keep = lane < m ? sorted[wave][lane] : 0ull;
        tau = m >= p.k ? sorted[wave][p.k - 1] : 0ull;
        mf_row_topk_sync<true>();
#pragma unroll
        for (int j = 0; j < (64 + IVF_PEND) / 64; ++j) mine[lane + 64 * j] = j == 0 ? keep : 0ull;
        pend = 0;
        mf_row_topk_sync<true>();
    };

    for (int64_t blk = b0 + wave; blk < b1; blk += MF_CELLS_NW) {
        unsigned long long word = ~0ull;
        if constexpr (ALLOW) {
            word = next_word;                                      // (blk is wave-uniform: b0 and the wave's number are)
            if (blk + MF_CELLS_NW < b1) next_word = mf_cells_allow_word(mask, blk + MF_CELLS_NW);
            if (word == 0ull) continue;                            // nothing of this block may enter: neither rows nor row_of are read
        }
        const f32x4* src = reinterpret_cast<const f32x4*>(p.blocked) + blk * (int64_t)CPR * 64 + lane;
        const int64_t orig = p.row_of[blk * 64 + lane];
        f32x4 rc[HALF];
        float acc = 0.f;
#pragma unroll
        for (int h0 = 0; h0 < CPR; h0 += HALF) {
#pragma unroll
            for (int j = 0; j < HALF; ++j) rc[j] = src[(int64_t)(h0 + j) * 64];
#pragma unroll
            for (int g = 0; g < HALF / 2; ++g) {
                const f32x4 a = rc[2 * g], b = rc[2 * g + 1];
                mf_const_f32 qv = qc + 4 * (h0 + 2 * g);         // wave-uniform address: scalar loads
#pragma unroll
                for (int t = 0; t < 4; ++t) {                      // k order of mf_dot_chain
                    acc = __builtin_fmaf(a[t], qv[t], acc);
                    acc = __builtin_fmaf(b[t], qv[4 + t], acc);
                }
            }
        }
        const unsigned grow = (unsigned)(p.idx_base + orig);       // the GLOBAL row: ties break by it whatever the permutation
        const unsigned long long key = orig >= 0 && (!ALLOW || mf_cells_allowed(word, lane)) ? mf_key_retrieval(acc, grow) : 0ull;
        bool pass = key > tau;
        if (p.excl_off) pass = mf_cells_admit(pass, grow, p.excl_idx, e0, e1, lane);
        const unsigned long long bal = __ballot(pass);
        if (bal) {
            if (pass) mine[64 + pend + __popcll(bal & below)] = key;
            pend += __popcll(bal);
            if (pend > IVF_PEND - 64) settle();                    // no room for another block's 64
        }
    }
    if (pend > 0) settle();                                        // (else the front is in order already: zeros, or the last settle)
    mf_row_topk_sync<true>();
    all[wave * 64 + lane] = mine[lane];
    __syncthreads();
    if (wave != 0) return;
    const int m = mf_row_topk<MF_CELLS_NW, true>(all, MF_CELLS_NW * 64, p.k, win[0], sorted[0]);
    if (lane < p.k) {
        const long long v = lane < m ? mf_cells_entry(sorted[0][lane]) : MF_PACKED_NONE;
        const int64_t g = (int64_t)probe * p.S + slice;
        p.out[(g * p.Q + q) * p.k + lane] = v;
    }
}
