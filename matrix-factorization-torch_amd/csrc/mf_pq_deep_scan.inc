// mf_pq_deep_scan.inc -- the scan kernel over quantised cells for deep lists, included from mf_ivf_deep.hip once per form with
//   MF_SCAN_KERNEL   the kernel's name: pq_deep_scan_kernel (mf_pq_scan_deep), pq_deep_scan_allow_kernel (mf_pq_scan_deep_allow)
//   MF_SCAN_ALLOW    false / true: a row enters a list only where the bit of its cell-ordered position is set in the query's
//                    mask (mf_cells.h), read by strips of 64 words as mf_pq_scan.inc does.  A wave whose word is 0 reads neither
//                    codes nor row_of, its key stays 0 -- and it still takes every barrier of the pass.
// Everything else is the same lines for both (text, not a template flag: mf_ivf_scan.inc).  Geometry, tables, scoring and keys
// are mf_pq_scan.inc's to the bit; the keeping is mf_ivf_deep_scan.inc's: the IVFD_BUF-key buffer, the kept part kp =
// ivfd_kept(R), the settle by ivfd_sort_desc when more than ivfd_capacity(kp) - kp - IVFD_PASS keys wait.
template <int M, int DSUB>
__global__ __launch_bounds__(IVFD_PASS) void MF_SCAN_KERNEL(PqScanParams p, int kp) {
    constexpr bool ALLOW = MF_SCAN_ALLOW;
    constexpr int D = M * DSUB;
    constexpr int U = M < 4 ? M : 4;           // code bytes per unit
    constexpr int NU = M / U;
    __shared__ float lut[M * 256];
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
    const float base = p.probe_scores[q * p.nprobe + probe];
    int64_t b0 = 0, b1 = 0;
    if (cell >= 0 && cell < p.C) {
        const int64_t c0 = p.cell_blk[cell], nb = p.cell_blk[cell + 1] - c0;
        b0 = c0 + nb * slice / p.S;
        b1 = c0 + nb * (slice + 1) / p.S;
    }
    int64_t e0 = 0, e1 = 0;
    if (p.excl_off) {
        e0 = p.excl_off[q];
        e1 = p.excl_off[q + 1];
    }
    // the words of the slice's blocks, 64 at a time and a strip ahead (mf_cells_allow_strip: the vector load, mf_pq_scan.inc)
    const unsigned long long* mask = nullptr;
    unsigned long long strip = 0ull, strip_next = 0ull;
    int64_t strip0 = b0;
    if constexpr (ALLOW) {
        mask = mf_cells_allow_mask(p.allow, q);
        strip = mf_cells_allow_strip(mask, b0, b1, lane);
        strip_next = mf_cells_allow_strip(mask, b0 + 64, b1, lane);
    }
    for (int i = tid; i < IVFD_BUF; i += IVFD_PASS) buf[i] = 0ull;
    if (b0 < b1) {                                                   // the query's tables: thread = codeword
        mf_const_f32 qc = (mf_const_f32)p.q + (size_t)q * D;
#pragma unroll 2                                                   // (the query's sub-vectors sit in scalar registers: mf_pq_scan.inc)
        for (int m = 0; m < M; ++m) {
            float b[DSUB];
            pq_load_sub<DSUB>(b, p.codebooks + ((size_t)m * 256 + tid) * DSUB);
            lut[m * 256 + tid] = pq_chain<DSUB>(qc + m * DSUB, b);
        }
    }
    __syncthreads();
    const int room = ivfd_capacity(kp) - kp - IVFD_PASS;             // waiting keys behind which another pass still fits
    unsigned long long tau = 0ull;             // the R-th best key once the buffer holds R: only a larger key matters
    int pend = 0;                              // keys waiting behind the kept ones (workgroup-uniform)
    // the R best of the kept and the waiting keys in descending order at the front, the rest cleared
    auto settle = [&]() {
        int n = IVFD_SORT_MIN;
        while (n < kp + pend) n <<= 1;
        ivfd_sort_desc(buf, n);
        tau = buf[p.R - 1];
        __syncthreads();
        for (int i = p.R + tid; i < n; i += IVFD_PASS) buf[i] = 0ull;   // (beyond n nothing was written)
        pend = 0;
        __syncthreads();
    };

    for (int64_t blk0 = b0; blk0 < b1; blk0 += MF_CELLS_NW) {         // (uniform trip count: barriers inside)
        const int64_t blk = blk0 + wave;
        unsigned long long key = 0ull;
        unsigned grow = 0u;
        unsigned long long word = ~0ull;
        if constexpr (ALLOW) {                                       // (blk0, blk and strip0 are wave-uniform)
            if (blk0 - strip0 >= 64) {                               // (blk0 - b0 is a multiple of four: a pass never straddles)
                strip0 += 64;
                strip = strip_next;
                strip_next = mf_cells_allow_strip(mask, strip0 + 64, b1, lane);
            }
            word = blk < b1 ? mf_cells_strip_word(strip, (int)(blk - strip0)) : 0ull;
        }
        if (blk < b1 && (!ALLOW || word != 0ull)) {
            const int64_t orig = p.row_of[blk * 64 + lane];
            float acc = base;
            if constexpr (U == 4) {
                const unsigned* src = reinterpret_cast<const unsigned*>(p.codes) + blk * (int64_t)NU * 64 + lane;
                unsigned w[NU];
#pragma unroll
                for (int u = 0; u < NU; ++u) w[u] = src[u * 64];
#pragma unroll
                for (int u = 0; u < NU; ++u) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc = acc + lut[(4 * u + b) * 256 + ((w[u] >> (8 * b)) & 255u)];
                }
            } else {
                const unsigned w = reinterpret_cast<const unsigned short*>(p.codes)[blk * 64 + lane];
                acc = acc + lut[w & 255u];
                acc = acc + lut[256 + (w >> 8)];
            }
            grow = (unsigned)(p.idx_base + orig);                    // the GLOBAL row: ties break by it
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
    long long* out = p.out + (g * p.Q + q) * p.R;
    for (int i = tid; i < p.R; i += IVFD_PASS) {
        const unsigned long long key = buf[i];
        out[i] = key != 0ull ? mf_cells_entry(key) : MF_PACKED_NONE;
    }
}
