// mf_loss_cols.h -- the column plan of the dense loss: sweep each DISTINCT item column once, weighted by its copy count.
//
// A Zipf batch repeats its popular items: of the 16,384 columns of the headline step ~10,700 are distinct.  Copies of a
// column have the same row bits (the tower gather is deterministic) and the same logQ, hence the same logit for every
// user; the three sweeps (mf_loss_dense.hip) then stream the N' distinct columns -- v'[k], |v'|^2, -logq', weight w[k] -- instead
// of all N.  The loss API takes v[N, d] and logq[N] as free inputs, so an id alone proves nothing: column j is a COPY iff
//     f = colfirst[j] != j,  the d floats of v[j] equal those of v[f] bit for bit,  and  -logq[j] equals -logq[f] bit for bit
// (the rule of the mining prefilter's rep[], mf_mine_bf.h).  Any other column is KEPT; a column whose id repeats with other
// values is simply kept (correct, just not merged).  Kept columns are compacted IN COLUMN ORDER (a scan, not the order
// atomics land in), the copy counts are integer adds (order-free), so the plan is the same bits on every run.
//
// Everything stays on the device: N' is never read by the host (no sync; a captured step replays it).  The split geometry
// of the three sweeps for N' is computed by the plan's last kernel with the SAME function the host uses for N
// (split_geometry below), and the sweeps are launched for the worst case and read their share from these words.
#pragma once

#include "mf_common.h"
#include "mf_lists.h"

// streamed axis of y_tiles tiles cut in nsplit ranges of tps tiles so that x_tiles x nsplit workgroups ~ target_blocks
__host__ __device__ static inline int split_want(int x_tiles, int y_tiles, int target_blocks) {
    int want = (target_blocks + x_tiles - 1) / x_tiles;
    if (want < 1) want = 1;
    if (want > y_tiles) want = y_tiles;
    return want;
}
__host__ __device__ static inline void split_geometry(int x_tiles, int y_tiles, int* nsplit, int* tps, int target_blocks) {
    const int want = split_want(x_tiles, y_tiles, target_blocks);
    *tps = (y_tiles + want - 1) / want;
    *nsplit = (y_tiles + *tps - 1) / *tps;
}

// device words of the plan (int32), at the very start of the loss workspace
enum { CG_NCOLS = 0, CG_NT, CG_NSF, CG_TPSF, CG_NSU, CG_TPSU, CG_NSV, CG_TPSV, CG_XBV, CG_WORDS = 16 };

struct ColsGeom {
    int ncols, nt;               // distinct columns; tiles the forward and dU stream (whole X blocks of dV: a multiple of NW)
    int nsf, tpsf, nsu, tpsu;    // forward / dU: item-range splits
    int nsv, tpsv, xbv;          // dV: user-range splits, and its X blocks
};
// BT / NT: user / item tiles (padded), NW: waves per workgroup, wgs_f / wgs_b: workgroups the forward / the backward sweeps
// aim at.  ncols = N gives what loss_ws computes for the uncompacted sweeps (mf_loss_plan).
// dV keeps X blocks of items, so ITS workgroup count moves with N': with the rounding-up of split_geometry, 84 X blocks
// (the headline batch) would get 7 splits = 588 workgroups on 512 slots -- a second round of 76 workgroups, slower than the
// 512 x 64 tiles it replaces.  Once the plan has removed an X block, dV therefore takes the most splits that still FIT the
// target (84 x 6 = 504 workgroups of 43 tiles).
__host__ __device__ static inline ColsGeom cols_geometry(int BT, int NT, int NW, int64_t ncols, int wgs_f, int wgs_b) {
    ColsGeom g;
    g.ncols = (int)ncols;
    g.xbv = (int)((ncols + 32 * NW - 1) / (32 * NW));
    g.nt = g.xbv * NW;
    split_geometry(BT / NW, g.nt, &g.nsf, &g.tpsf, wgs_f);
    split_geometry(BT / NW, g.nt, &g.nsu, &g.tpsu, wgs_b);
    split_geometry(g.xbv, BT, &g.nsv, &g.tpsv, wgs_b);
    if (g.xbv < NT / NW && g.xbv * g.nsv > wgs_b) split_geometry(g.xbv, BT, &g.nsv, &g.tpsv, wgs_b / g.xbv * g.xbv);
    return g;
}
// what is LAUNCHED, whatever N' turns out to be: splits of the forward and of dU (the most any ncols <= N can ask for), and
// the linear grid of dV (x blocks x splits < wgs_b + x blocks for every ncols)
struct ColsLaunch {
    int grid_f, grid_u, grid_v;
};
static inline ColsLaunch cols_launch(int BT, int NT, int NW, int wgs_f, int wgs_b) {
    ColsLaunch l;
    l.grid_f = split_want(BT / NW, NT, wgs_f);
    l.grid_u = split_want(BT / NW, NT, wgs_b);
    l.grid_v = wgs_b + NT / NW;
    return l;
}

#ifdef __HIPCC__

// One workgroup per tile of 32 columns, 32 lanes per column (16 bytes of the row each): kept[j] = 1 unless column j is a
// copy (or padding); tcnt[tile] = kept columns of the tile.
template <int D>
__global__ __launch_bounds__(1024) void cols_mark_kernel(const float* __restrict__ v, const float* __restrict__ nlogq,
                                                         const int32_t* __restrict__ colfirst, int64_t N,
                                                         int32_t* __restrict__ kept, int32_t* __restrict__ tcnt) {
    static_assert(D == 128, "32 lanes of 16 bytes per row");
    __shared__ int sk[32];
    const int g = threadIdx.x >> 5, c = threadIdx.x & 31;
    const int64_t j = (int64_t)blockIdx.x * 32 + g;
    int32_t f = -1;
    if (j < N) f = colfirst[j];
    const bool cand = j < N && f >= 0 && f != j;
    bool same = true;
    if (cand) {
        const uint4 a = reinterpret_cast<const uint4*>(v + j * D)[c], b = reinterpret_cast<const uint4*>(v + (int64_t)f * D)[c];
        same = a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w &&
               __builtin_bit_cast(unsigned, nlogq[j]) == __builtin_bit_cast(unsigned, nlogq[f]);
    }
    const unsigned long long m = __ballot(same);                    // (every lane of the wave is here)
    const bool all_same = (unsigned)(m >> (32 * (mf_lane() >> 5))) == 0xFFFFFFFFu;
    const bool copy = cand && all_same;
    const int keep = (j < N && !copy) ? 1 : 0;
    if (c == 0) {
        kept[j] = keep;
        sk[g] = keep;
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        const unsigned long long kb = __ballot(sk[threadIdx.x] != 0);
        if (threadIdx.x == 0) tcnt[blockIdx.x] = __popcll(kb);
    }
}

struct ColsPack {
    const float *v, *nv, *nlogq;
    const int32_t *colfirst, *kept, *tcnt;
    int64_t N, Np;
    int NT, BT, NW, wgs_f, wgs_b;
    int32_t *rank, *cfirst, *geo, *ccnt;
    float *cnv, *clq;
};
// One workgroup per 1024 columns: its base = kept columns before it (the tile counts: a sum, the same on every run), then
// a block scan in column order.  Kept column j -> slot k: rank[j] = k, first'[k] = colfirst[j], |v|^2, -logq.  A copy keeps
// ~(its first column) in rank[j]: the epilogue takes rank[first] (the first column of an id is always kept), and adds 1 to
// its first column's count -- integer adds, gathered per workgroup in an LDS table first (2048 slots for <= 1024 keys: never
// full): the ~700 copies of a Zipf batch's most popular item are 16 global atomics on its word instead of 700 queued at one
// L2 channel.  Scalar slots from N' up to the padded end: first' = -1 (masked for every user), 0.  Workgroup 0 writes the
// geometry words.  cols_rows_kernel, behind it, moves the rows and turns the counts into weights.
template <int D>
__global__ __launch_bounds__(1024) void cols_pack_kernel(ColsPack p) {
    static_assert(D == 128, "32 lanes of 16 bytes per row");
    __shared__ int hkey[2048], hcnt[2048];
    const int tid = threadIdx.x;
    hkey[tid] = -1; hkey[tid + 1024] = -1; hcnt[tid] = 0; hcnt[tid + 1024] = 0;
    const int64_t j0 = (int64_t)blockIdx.x * 1024, j = j0 + tid;
    int64_t s[2] = {0, 0}, tot[2];
    for (int t = tid; t < p.NT; t += 1024) {
        const int n = p.tcnt[t];
        s[1] += n;
        if (t < (int)blockIdx.x * 32) s[0] += n;
    }
    block_excl_scan<1024, 2>(s, tot);
    const int64_t base = tot[0], ncols = tot[1];
    const int keep = j < p.Np ? p.kept[j] : 0;
    int64_t pos[1] = {keep}, ptot[1];
    block_excl_scan<1024, 1>(pos, ptot);
    const int64_t k = base + pos[0];
    if (keep) {
        p.rank[j] = (int32_t)k;
        p.cfirst[k] = p.colfirst[j];
        p.cnv[k] = p.nv[j];
        p.clq[k] = p.nlogq[j];
    } else if (j < p.N) {                         // a copy (block_excl_scan's barriers stand between the table's clearing and here)
        const int f = p.colfirst[j];
        p.rank[j] = ~f;
        unsigned h = ((unsigned)f * 2654435761u) >> 21;           // 11 bits
        for (int probe = 0; probe < 2048; ++probe) {
            const int old = atomicCAS(&hkey[h], -1, f);
            if (old == -1 || old == f) { atomicAdd(&hcnt[h], 1); break; }
            h = (h + 1) & 2047u;
        }
    }
    if (j >= ncols && j < p.Np) {                 // (slot j: no kept column lands at or beyond N')
        p.cfirst[j] = -1;
        p.cnv[j] = 0.f; p.clq[j] = 0.f;
    }
    __syncthreads();
    for (int q = tid; q < 2048; q += 1024)
        if (hkey[q] >= 0) atomicAdd(&p.ccnt[hkey[q]], hcnt[q]);
    if (blockIdx.x == 0 && tid == 0) {
        const ColsGeom q = cols_geometry(p.BT, p.NT, p.NW, ncols, p.wgs_f, p.wgs_b);
        p.geo[CG_NCOLS] = q.ncols; p.geo[CG_NT] = q.nt;
        p.geo[CG_NSF] = q.nsf; p.geo[CG_TPSF] = q.tpsf; p.geo[CG_NSU] = q.nsu; p.geo[CG_TPSU] = q.tpsu;
        p.geo[CG_NSV] = q.nsv; p.geo[CG_TPSV] = q.tpsv; p.geo[CG_XBV] = q.xbv;
    }
}

// One workgroup per tile of 32 columns, 32 lanes per row: kept column j's row goes to its slot, slot j from N' up is a zero
// row, and slot k's weight is 1 + the copies counted on its column (0 from N' up).
template <int D>
__global__ __launch_bounds__(1024) void cols_rows_kernel(const float* __restrict__ v, const int32_t* __restrict__ rank,
                                                         const int32_t* __restrict__ ccnt, const int32_t* __restrict__ geo,
                                                         int64_t N, float* __restrict__ cv, float* __restrict__ cw) {
    static_assert(D == 128, "32 lanes of 16 bytes per row");
    const int g = threadIdx.x >> 5, c = threadIdx.x & 31;
    const int64_t j = (int64_t)blockIdx.x * 32 + g;          // (the grid covers the padded columns exactly)
    const int ncols = geo[CG_NCOLS];
    const int32_t k = j < N ? rank[j] : -1;
    if (k >= 0) {
        reinterpret_cast<uint4*>(cv + (int64_t)k * D)[c] = reinterpret_cast<const uint4*>(v + j * D)[c];
        if (c == 0) cw[k] = (float)(1 + ccnt[j]);
    }
    if (j >= ncols) {
        reinterpret_cast<uint4*>(cv + j * D)[c] = uint4{0u, 0u, 0u, 0u};
        if (c == 0) cw[j] = 0.f;
    }
}

#endif  // __HIPCC__
