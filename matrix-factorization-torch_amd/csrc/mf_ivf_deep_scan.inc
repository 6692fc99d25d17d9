// mf_ivf_deep_scan.inc -- the scan kernel of mf_ivf_deep.hip, included once per form with
//   MF_SCAN_KERNEL   the kernel's name: ivf_scan_deep_kernel (mf_ivf_scan_deep), ivf_scan_deep_allow_kernel (mf_ivf_scan_deep_allow)
//   MF_SCAN_ALLOW    false / true: a row enters a list only where the bit of its cell-ordered position is set in the query's
//                    mask (mf_cells.h).  A wave whose word is 0 reads neither rows nor row_of, its key stays 0 -- and it still
//                    takes every barrier of the pass.
// Everything else is the same lines for both (text, not a template flag: mf_ivf_scan.inc).  Geometry, scoring and keys are
// mf_ivf_scan.inc's; the keeping is the workgroup's (mf_pq_scan.inc), with the buffer and the sort of mf_ivf_deep.hip.
template <int D>
__global__ __launch_bounds__(IVFD_PASS) void MF_SCAN_KERNEL(IvfDeepParams p) {
    constexpr bool ALLOW = MF_SCAN_ALLOW;
    constexpr int CPR = D / 4;
    constexpr int HALF = CPR > 32 ? 32 : CPR;                  // chunks held in registers at once
    __shared__ unsigned long long buf[IVFD_BUF];               // the kp best keys so far [0, kp), then the waiting ones
    __shared__ int cnt[MF_CELLS_NW];
    const int tid = threadIdx.x, lane = mf_lane(), wave = mf_wave_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    // blockIdx.x = (q * nprobe + probe) * S + slice: everything here is workgroup-uniform (mf_ivf.hip has the same lines: mf_cells.h)
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
    // the word of the wave's next block is asked for a block ahead (mf_ivf_scan.inc)
    const unsigned long long* mask = nullptr;
    unsigned long long next_word = 0ull;
    if constexpr (ALLOW) {
        mask = mf_cells_allow_mask(p.allow, q);
        if (b0 + wave < b1) next_word = mf_cells_allow_word(mask, b0 + wave);
    }
    const int kp = p.kp, room = ivfd_capacity(kp) - kp - IVFD_PASS;     // waiting keys behind which another pass still fits
    for (int i = tid; i < IVFD_BUF; i += IVFD_PASS) buf[i] = 0ull;
    __syncthreads();
    unsigned long long tau = 0ull;             // the k-th best key once the buffer holds k: only a larger key matters
    int pend = 0;                              // keys waiting behind the kept ones (workgroup-uniform)
    // the k best of the kept and the waiting keys in descending order at the front, the rest cleared
    auto settle = [&]() {
        int n = IVFD_SORT_MIN;
        while (n < kp + pend) n <<= 1;
        ivfd_sort_desc(buf, n);
        tau = buf[p.k - 1];
        __syncthreads();
        for (int i = p.k + tid; i < n; i += IVFD_PASS) buf[i] = 0ull;   // (beyond n nothing was written)
        pend = 0;
        __syncthreads();
    };

    for (int64_t blk0 = b0; blk0 < b1; blk0 += MF_CELLS_NW) {         // (uniform trip count: barriers inside)
        const int64_t blk = blk0 + wave;
        unsigned long long key = 0ull;
        unsigned grow = 0u;
        unsigned long long word = ~0ull;
        if constexpr (ALLOW) {
            word = next_word;                                      // (blk is wave-uniform: blk0 and the wave's number are)
            next_word = blk + MF_CELLS_NW < b1 ? mf_cells_allow_word(mask, blk + MF_CELLS_NW) : 0ull;
            if (blk >= b1) word = 0ull;
        }
        if (blk < b1 && (!ALLOW || word != 0ull)) {                  // (else nothing of this block may enter: neither rows nor row_of are read)
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
            grow = (unsigned)(p.idx_base + orig);                    // the GLOBAL row: ties break by it whatever the permutation
            key = orig >= 0 && (!ALLOW || mf_cells_allowed(word, lane)) ? mf_key_retrieval(acc, grow) : 0ull;
        }
        bool pass = key > tau;
        if (p.excl_off) pass = mf_cells_admit(pass, grow, p.excl_idx, e0, e1, lane);
        const unsigned long long bal = __ballot(pass);
        if (lane == 0) cnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < MF_CELLS_NW; ++w) {
            const int c = cnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (pass) buf[kp + pend + before + __popcll(bal & below)] = key;
        pend += total;
        __syncthreads();
        if (pend > room) settle();                                   // no room for another pass's IVFD_PASS keys
    }
    if (pend > 0) settle();                                          // (else the front is in order already: zeros, or the last settle)
    const int64_t g = (int64_t)probe * p.S + slice;
    long long* out = p.out + (g * p.Q + q) * p.k;
    for (int i = tid; i < p.k; i += IVFD_PASS) {
        const unsigned long long key = buf[i];
        out[i] = key != 0ull ? mf_cells_entry(key) : MF_PACKED_NONE;
    }
}
