// mf_logq.hip -- streaming logQ: the per-step inclusion rate of an id, estimated from the batches themselves
// (Yi et al. 2019, "Sampling-bias-corrected neural modeling", Algorithms 2 and 3).  Spec: include/mf_hip.h, DESIGN.md 4.
//
// State per bucket: last_seen (int32 step, 0 = never) and gap (fp32 moving average of the steps between two sightings,
// 0 = never).  An update is ONE launch: one lane per (id, hash) claims its bucket with an integer atomicExch of the step
// number.  The lane that gets a value other than t back is the first of this step to reach the bucket -- whichever copy
// that is, what it gets back is the step of the PREVIOUS sighting -- and it alone reads and writes gap (and the table
// entry) with plain loads and stores.  Nobody reads what another lane of the launch wrote, so the launch needs no fence,
// no float atomic and no wait; the read-out of the rows runs behind the kernel boundary.
#include <math.h>

#include "mf_common.h"

// Copies of one bucket inside a wave: up to `peel` times the wave takes the bucket of its first pending lane, every lane
// that holds it stands down and that first lane alone goes to memory.  The hottest ids of a Zipf batch come hundreds of
// times and one word serves only so many atomics per microsecond; what is left after the rounds goes lane by lane.  Only
// speed depends on it: the atomicExch decides the claim whoever asks.
static int g_logq_peel = 4;
extern "C" void mf_logq_set_peel(int rounds) { g_logq_peel = rounds < 0 ? 0 : (rounds > 8 ? 8 : rounds); }

__device__ __forceinline__ int64_t logq_slot(int64_t id, int j, int hashes, unsigned long long seed, int64_t n_buckets) {
    if (hashes == 0) return (id >= 0 && id < n_buckets) ? id : -1;
    return id >= 0 ? (int64_t)j * n_buckets + mf_hash_bucket(id, j, seed, n_buckets) : -1;
}

// grid (ids / 256, max(hashes, 1)): blockIdx.y is the hash
__global__ __launch_bounds__(256) void logq_update_kernel(int32_t* __restrict__ last_seen, float* __restrict__ gap, int64_t n_buckets,
                                                          int hashes, unsigned long long seed, const int64_t* __restrict__ ids,
                                                          int64_t n, int64_t t_host, const int64_t* __restrict__ t_dev, float alpha,
                                                          float* __restrict__ table, int peel) {
    const int64_t t64 = t_dev ? *t_dev : t_host;
    if (t64 < 1 || t64 > 0x7FFFFFFFll) return;                 // (a device counter outside the range: nothing is touched)
    const int t = (int)t64;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t slot = i < n ? logq_slot(ids[i], (int)blockIdx.y, hashes, seed, n_buckets) : -1;
    bool pending = slot >= 0, claim = false;
    for (int r = 0; r < peel; ++r) {
        const unsigned long long m = __ballot(pending);
        if (!m) break;
        const int lead = __builtin_ctzll(m);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)slot, lead);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)slot >> 32), lead);
        if (pending && slot == (int64_t)(((unsigned long long)hi << 32) | lo)) {
            pending = false;
            claim = mf_lane() == lead;
        }
    }
    if (!(claim || pending)) return;
    const int old = atomicExch(&last_seen[slot], t);
    if (old == t) return;                                      // another copy of the bucket came first, or t was here already
    const float g = (float)(t - old);                          // v_cvt_f32_i32: round to nearest even
    float d = g;
    if (old != 0) {
        const float keep = 1.0f - alpha;
        d = keep * gap[slot] + alpha * g;                      // (-ffp-contract=off: two products, one sum, each rounded)
    }
    gap[slot] = d;
    if (table) table[slot] = -logf(d);
}

// out[i] = -log(largest gap among the id's buckets); 0 for an id outside the domain or with a bucket never seen
__global__ __launch_bounds__(256) void logq_read_kernel(const float* __restrict__ gap, int64_t n_buckets, int hashes,
                                                        unsigned long long seed, const int64_t* __restrict__ ids, int64_t n,
                                                        float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids[i];
    const int hh = hashes > 0 ? hashes : 1;
    float d = 0.0f;
    bool seen = true;
    for (int j = 0; j < hh; ++j) {
        const int64_t slot = logq_slot(id, j, hashes, seed, n_buckets);
        const float x = slot >= 0 ? gap[slot] : 0.0f;
        seen = seen && x != 0.0f;
        d = MF_FMAXF(d, x);
    }
    out[i] = seen ? -logf(d) : 0.0f;
}

static int logq_check(const char* who, const void* gap, int64_t n_buckets, int num_hashes, const int64_t* ids, int64_t n) {
    if (!gap || (!ids && n != 0) || n < 0 || n_buckets < 1 || num_hashes < 0 || num_hashes > 4)
        return mf_set_error(MF_EINVAL, "%s: bad argument", who);
    return MF_OK;
}

static int logq_grid(const char* who, int64_t n, int64_t n_buckets, unsigned* blocks) {
    if (n_buckets >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "%s: n_buckets = %lld does not fit 31 bits", who, (long long)n_buckets);
    const int64_t b = (n + 255) / 256;
    if (b >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "%s: n = %lld ids exceed one launch", who, (long long)n);
    *blocks = (unsigned)b;
    return MF_OK;
}

extern "C" int mf_logq_update(int32_t* last_seen, float* gap, int64_t n_buckets, int num_hashes, uint64_t seed, const int64_t* ids,
                              int64_t n, int64_t t, const int64_t* t_dev, float alpha, float* logq_table, float* out_logq,
                              mf_stream_t stream) {
    const char* who = "mf_logq_update";
    if (!last_seen) return mf_set_error(MF_EINVAL, "%s: bad argument", who);
    if (int rc = logq_check(who, gap, n_buckets, num_hashes, ids, n)) return rc;
    if (!(alpha > 0.0f && alpha <= 1.0f)) return mf_set_error(MF_EINVAL, "%s: alpha = %g outside (0, 1]", who, (double)alpha);
    if (!t_dev && t < 1) return mf_set_error(MF_EINVAL, "%s: step t = %lld < 1", who, (long long)t);
    if (logq_table && num_hashes > 0) return mf_set_error(MF_EINVAL, "%s: a logq_table needs direct mode (num_hashes = 0)", who);
    if (!t_dev && t >= (1ll << 31)) return mf_set_error(MF_ENOTSUP, "%s: step t = %lld does not fit 31 bits", who, (long long)t);
    unsigned blocks = 0;
    if (int rc = logq_grid(who, n, n_buckets, &blocks)) return rc;
    if (n == 0) return MF_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    logq_update_kernel<<<dim3(blocks, (unsigned)(num_hashes > 0 ? num_hashes : 1)), 256, 0, s>>>(
        last_seen, gap, n_buckets, num_hashes, seed, ids, n, t, t_dev, alpha, logq_table, g_logq_peel);
    if (out_logq) logq_read_kernel<<<dim3(blocks), 256, 0, s>>>(gap, n_buckets, num_hashes, seed, ids, n, out_logq);
    return mf_check_launch(who);
}

extern "C" int mf_logq_lookup(const float* gap, int64_t n_buckets, int num_hashes, uint64_t seed, const int64_t* ids, int64_t n,
                              float* out_logq, mf_stream_t stream) {
    const char* who = "mf_logq_lookup";
    if (int rc = logq_check(who, gap, n_buckets, num_hashes, ids, n)) return rc;
    if (!out_logq && n != 0) return mf_set_error(MF_EINVAL, "%s: bad argument", who);
    unsigned blocks = 0;
    if (int rc = logq_grid(who, n, n_buckets, &blocks)) return rc;
    if (n == 0) return MF_OK;
    logq_read_kernel<<<dim3(blocks), 256, 0, static_cast<hipStream_t>(stream)>>>(gap, n_buckets, num_hashes, seed, ids, n, out_logq);
    return mf_check_launch(who);
}
