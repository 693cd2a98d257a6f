// 3-D marker-in-cell: tracer->grid, grid->tracer, RK4 advection and the resident tracer state of a pl3_ctx.
// The dimension-by-dimension extension of pylamp_trac.py:30-388 (the reference is 2-D only); conventions: positions (n,3) in
// [z, x, y] order, tracer fields with the 2-D columns of pylamp_const.py, grid arrays C-order (nz, nx, ny).  One rank only.
//
// Tracer -> grid is a GATHER: the tracers are sorted by cell (counting sort, made stable by ordering every cell's slice by the
// previous index), the start offset of every cell is kept, and each target node sums the tracers of the cells around it in a fixed
// order.  No floating-point atomics anywhere, so a scatter is bitwise the same from run to run.  Whether a tracer contributes to a
// node is decided by the tracer's own cell on the TARGET node set (the reference's regular-grid formula); the sort cells only
// bound the search, so a tracer on an exact cell face cannot be lost or counted twice.
//
// Grid -> tracer: out-of-grid tracers get defval in EVERY column.  This deliberately does not copy the 2-D quirk of
// pylamp_trac.py:83-156 (which leaves vz extrapolated under VELDIV): it has no meaning with three components.
#include "pl_internal.h"
#include "pl_mic3.h"
#include "pl_reduce3.h"
#include "pl_step3.h"
#include "pl_walls3.h"
#include <algorithm>
#include <cmath>

#define M3_MAXF 8
#define M3_NFTRAC 13
#define M3_ID 12
enum { M3_RHO = 0, M3_ETA = 1, M3_TMP = 3, M3_HCD = 4, M3_HCP = 5, M3_RH0 = 6, M3_ALP = 7, M3_ACE = 9, M3_ET0 = 10 };
#define M3_GASR 8.31446

// one axis of a node set: n coordinates c[].  Regular grids: cell = floor((n-1)(x - c0)/L) (pylamp_trac.py:42-47,222-227).  With
// the per-axis search (pl3_mic_set_search) the cell comes from comparisons with c[]: cl = c[n-1], and bin[] holds, for nbin equal
// buckets over [c0, cl], a cell that is not above the cell of any point of the bucket (binv = nbin / (cl - c0)); nbin = 0 without it.
struct M3Axis { int n; double c0, L, h0, h1; const double* c; double cl, binv; int nbin; const int* bin; };
struct M3Grid { M3Axis a[3]; };

__device__ inline double m3_cellf(const M3Axis& a, double p) { return floor((double)(a.n - 1) * (p - a.c0) / a.L); }
// coordinate of node i of the auto-extended node set (pylamp_trac.py:207-220): beyond the ends it continues with the end spacing
__device__ inline double m3_coord(const M3Axis& a, int i) {
    if (i < 0) return a.c0 + (double)i * a.h0;
    if (i > a.n - 1) return a.c[a.n - 1] + (double)(i - (a.n - 1)) * a.h1;
    return a.c[i];
}
__device__ inline int m3_sort_cell(const M3Axis& a, double p) {
    const double f = m3_cellf(a, p);
    return f >= (double)(a.n - 2) ? a.n - 2 : (f > 0.0 ? (int)f : 0);       // clamped into the node set (NaN -> 0)
}

// Search mode, c0 <= p < cl: the i with c[i] <= p < c[i+1].  The bucket is clamped as a double before the conversion (NaN, inf and
// huge values never index the table); from the bucket's entry the walk goes up while p >= c[i+1] and then down while p < c[i], so the
// answer rests on the comparisons alone and the table can only shorten the walk.  Both loops are bounded by n.  lo, hi = c[i], c[i+1]
// of the answer.  The three coordinates from the entry on are loaded together, so that the usual cases -- no step, or the one step
// up of a point whose bucket starts on a cell face -- cost two dependent loads (table, coordinates) and no more.
__device__ inline int m3_search_cell(const M3Axis& a, double p, double& lo, double& hi) {
    const double b = (p - a.c0) * a.binv;
    int i = a.bin[b >= (double)(a.nbin - 1) ? a.nbin - 1 : (b > 0.0 ? (int)b : 0)];
    lo = a.c[i]; hi = a.c[i + 1];
    const double h2 = a.c[min(i + 2, a.n - 1)];
    if (i < a.n - 2 && p >= hi) { i++; lo = hi; hi = h2; }
    for (int s = 0; s < a.n && i < a.n - 2 && p >= hi; s++) { i++; lo = hi; hi = a.c[i + 1]; }
    for (int s = 0; s < a.n && i > 0 && p < lo; s++) { i--; hi = lo; lo = a.c[i]; }
    return i;
}
template <bool SEARCH>
__device__ inline int m3_sort_cell_of(const M3Axis& a, double p) {
    if constexpr (!SEARCH) return m3_sort_cell(a, p);
    else {
        if (!(p >= a.c0)) return 0;                                         // below the set, or NaN
        double lo, hi;
        return p >= a.cl ? a.n - 2 : m3_search_cell(a, p, lo, hi);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// sort by cell
// ---------------------------------------------------------------------------------------------------------------------
// position of tracer t along axis a is x[a][t * xs]: xs = 1 for the resident SoA columns, 3 for a host (n,3) array
struct M3Pos { const double* x[3]; long long xs; };

// DEL (pl3_mic_set_deletion): a tracer with x_d <= 0 or x_d >= the last coordinate on any axis (NaN compares false and stays) gets
// the key m = the number of cells, a trash bucket behind the last cell.  The bucket is counted with ONE add per wave (ballot and
// popcount of the leaving lanes): when a whole layer leaves, tens of thousands of lanes would otherwise queue on one address.
template <bool SEARCH, bool DEL>
__global__ __launch_bounds__(256) void k_m3_key(long long n, M3Pos p, M3Grid s, int* __restrict__ key, int* __restrict__ count) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    if constexpr (DEL) {
        bool out = false;
#pragma unroll
        for (int d = 0; d < 3; d++) { const double x = p.x[d][t * p.xs]; out = out || x <= 0.0 || x >= s.a[d].cl; }
        const unsigned long long leaving = __ballot(out);
        if (out) {
            const int m = (s.a[0].n - 1) * (s.a[1].n - 1) * (s.a[2].n - 1);
            key[t] = m;
            if ((int)(threadIdx.x & 63) == __ffsll((long long)leaving) - 1) atomicAdd(&count[m], __popcll(leaving));
            return;
        }
    }
    const int ci = m3_sort_cell_of<SEARCH>(s.a[0], p.x[0][t * p.xs]), cj = m3_sort_cell_of<SEARCH>(s.a[1], p.x[1][t * p.xs]),
              ck = m3_sort_cell_of<SEARCH>(s.a[2], p.x[2][t * p.xs]);
    const int c = (ci * (s.a[1].n - 1) + cj) * (s.a[2].n - 1) + ck;
    key[t] = c;
    atomicAdd(&count[c], 1);                      // integer: the counts do not depend on the order of arrival
}
// Exclusive prefix sum over the cells in three plain launches, reduce-then-scan, so that no workgroup ever waits on another one:
// (1) k_m3_tile_sums: every workgroup sums its tile of M3_TILE cells, (2) k_m3_scan_sums: ONE workgroup scans the tile sums (a
// thousand of them for two million cells), (3) k_m3_scan_tiles: every workgroup scans its tile again, starting from its base.
// What is scanned is computed from the count array on the fly, so the scans of a refill share the pass (NS = 3):
//   0: count + deficit -> start (every cell's slice with the room for its new tracers behind the residents) and cursor,
//   1: deficit         -> ordinal of the cell's first new tracer among all new ones,
//   2: deficient flag  -> rank of the cell among the deficient ones = its slot in the compacted list the injection works from;
// 1 and 2 are only stored for the deficient cells, in that list.  NS = 1 scans the counts alone (no refill).  Integers
// throughout: the result does not depend on the tiling.
#define M3_TILE 2048
#define M3_NOCELL 0x7fffffff                      // padding behind the last cell: counts as nothing in every sum
struct M3Need { int dens, dmin; };               // a cell with count < dmin receives dens - count new tracers (dmin <= 0: none)
struct M3Totals { int v[6]; double maxid; };     // sums of 0..2, empty cells, smallest count; largest TR__ID (when asked for)

__device__ inline int m3_need(int c, M3Need r) { return c < r.dmin ? r.dens - c : 0; }
__device__ inline void m3_load8(int m, const int* __restrict__ cnt, long long base, int v[8]) {
    if (base + 8 <= (long long)m) {
        const int4 a = *(const int4*)(cnt + base), b = *(const int4*)(cnt + base + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else
        for (int k = 0; k < 8; k++) v[k] = base + k < (long long)m ? cnt[base + k] : M3_NOCELL;
}
template <int NS>
__device__ inline void m3_thread_sums(const int v[8], M3Need r, int s[NS]) {
    for (int a = 0; a < NS; a++) s[a] = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (v[k] == M3_NOCELL) continue;
        const int need = NS > 1 ? m3_need(v[k], r) : 0;
        s[0] += v[k] + need;
        if constexpr (NS > 1) { s[1] += need; s[2] += need > 0 ? 1 : 0; }
    }
}
// exclusive prefix of s[] over the 256 threads of the workgroup (in place)
template <int NS>
__device__ inline void m3_block_exscan(int s[NS]) {
    __shared__ int wsum[NS][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc[NS];
    for (int a = 0; a < NS; a++) {
        int x = s[a];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
        inc[a] = x;
        if (lane == 63) wsum[a][w] = x;
    }
    __syncthreads();
    for (int a = 0; a < NS; a++) {
        int b = 0;
        for (int q = 0; q < w; q++) b += wsum[a][q];
        s[a] = b + inc[a] - s[a];
    }
}
// bsum[a * nb + tile]: a < NS the tile sums; NS = 3: a = 3 the empty cells and a = 4 the smallest count of the tile
template <int NS>
__global__ __launch_bounds__(256) void k_m3_tile_sums(int m, const int* __restrict__ cnt, M3Need r, int nb, int* __restrict__ bsum) {
    constexpr int NR = NS > 1 ? NS + 2 : NS;
    __shared__ int sh[NR][4];
    int v[8], s[NR];
    m3_load8(m, cnt, (long long)blockIdx.x * M3_TILE + threadIdx.x * 8, v);
    m3_thread_sums<NS>(v, r, s);
    if constexpr (NS > 1) {
        s[NS] = 0; s[NS + 1] = M3_NOCELL;
#pragma unroll
        for (int k = 0; k < 8; k++) { s[NS] += v[k] == 0 ? 1 : 0; s[NS + 1] = min(s[NS + 1], v[k]); }
    }
    for (int a = 0; a < NR; a++) {
        int x = s[a];
        const bool mn = NS > 1 && a == NS + 1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const int y = __shfl_down(x, o, 64); x = mn ? min(x, y) : x + y; }
        if ((threadIdx.x & 63) == 0) sh[a][threadIdx.x >> 6] = x;
    }
    __syncthreads();
    if (threadIdx.x < NR) {
        const int a = threadIdx.x;
        const bool mn = NS > 1 && a == NS + 1;
        int x = sh[a][0];
        for (int q = 1; q < 4; q++) x = mn ? min(x, sh[a][q]) : x + sh[a][q];
        bsum[(size_t)a * nb + blockIdx.x] = x;
    }
}
// one workgroup: the tile sums become the tiles' bases (exclusive, in place), the totals go to tot; with idpart the largest
// tracer ID is finished from the partial maxima of k_m3_max
template <int NS>
__global__ __launch_bounds__(1024) void k_m3_scan_sums(int nb, int* __restrict__ bsum, M3Totals* __restrict__ tot, const double* __restrict__ idpart, int nid) {
    __shared__ int part[1024];
    __shared__ double dpart[16];
    const int tid = threadIdx.x, chunk = (nb + 1023) / 1024, b = min(tid * chunk, nb), e = min(b + chunk, nb);
    for (int a = 0; a < NS; a++) {
        int* x = bsum + (size_t)a * nb;
        int s = 0;
        for (int i = b; i < e; i++) s += x[i];
        part[tid] = s;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int u = tid >= d ? part[tid - d] : 0;
            __syncthreads();
            part[tid] += u;
            __syncthreads();
        }
        int run = part[tid] - s;
        for (int i = b; i < e; i++) { const int u = x[i]; x[i] = run; run += u; }
        if (tid == 1023) tot->v[a] = part[1023];
        __syncthreads();
    }
    if constexpr (NS > 1) {
        for (int a = NS; a < NS + 2; a++) {
            const bool mn = a == NS + 1;
            const int* x = bsum + (size_t)a * nb;
            int s = mn ? M3_NOCELL : 0;
            for (int i = b; i < e; i++) s = mn ? min(s, x[i]) : s + x[i];
            part[tid] = s;
            __syncthreads();
            for (int d = 512; d > 0; d >>= 1) {
                if (tid < d) part[tid] = mn ? min(part[tid], part[tid + d]) : part[tid] + part[tid + d];
                __syncthreads();
            }
            if (tid == 0) tot->v[a] = part[0];
            __syncthreads();
        }
    }
    if (idpart) {
        double mx = -INFINITY;
        for (int i = tid; i < nid; i += 1024) mx = fmax(mx, idpart[i]);
        r3_wave(R3_MAX, mx);
        if ((tid & 63) == 0) dpart[tid >> 6] = mx;
        __syncthreads();
        if (tid == 0) { for (int q = 1; q < 16; q++) mx = fmax(mx, dpart[q]); tot->maxid = mx; }
    }
}
template <int NS>
__global__ __launch_bounds__(256) void k_m3_scan_tiles(int m, const int* __restrict__ cnt, M3Need r, int nb, const int* __restrict__ bsum,
                                                       const M3Totals* __restrict__ tot, int* __restrict__ start, int* __restrict__ cursor,
                                                       int* __restrict__ list, int* __restrict__ loff, int trash) {
    const long long base = (long long)blockIdx.x * M3_TILE + threadIdx.x * 8;
    int v[8], s[NS], o[8];
    m3_load8(m, cnt, base, v);
    m3_thread_sums<NS>(v, r, s);
    m3_block_exscan<NS>(s);
    for (int a = 0; a < NS; a++) s[a] += bsum[(size_t)a * nb + blockIdx.x];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        o[k] = s[0];
        if (v[k] == M3_NOCELL) continue;
        const int need = NS > 1 ? m3_need(v[k], r) : 0;
        s[0] += v[k] + need;
        if constexpr (NS > 1) if (need > 0) { list[s[2]] = (int)(base + k); loff[s[2]] = s[1]; s[1] += need; s[2]++; }
    }
    if (base + 8 <= (long long)m) {
        const int4 a = make_int4(o[0], o[1], o[2], o[3]), b = make_int4(o[4], o[5], o[6], o[7]);
        *(int4*)(start + base) = a; *(int4*)(start + base + 4) = b;
        *(int4*)(cursor + base) = a; *(int4*)(cursor + base + 4) = b;
    } else
        for (int k = 0; k < 8; k++) if (base + k < (long long)m) { start[base + k] = o[k]; cursor[base + k] = o[k]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) { start[m] = tot->v[0]; if (trash) cursor[m] = tot->v[0]; }      // the trash bucket's slice starts behind the last cell
}
__global__ __launch_bounds__(256) void k_m3_place(long long n, const int* __restrict__ key, int* __restrict__ cursor, int* __restrict__ perm) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    perm[atomicAdd(&cursor[key[t]], 1)] = (int)t;
}
// k_m3_place of a deleting sort: the leavers (key == trash) go behind the last cell.  They all want the same cursor, so a wave takes
// its slots with one add and hands them out by lane rank
__global__ __launch_bounds__(256) void k_m3_place_del(long long n, const int* __restrict__ key, int* __restrict__ cursor, int* __restrict__ perm, int trash) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int c = key[t];
    const bool out = c == trash;
    const unsigned long long leaving = __ballot(out);
    if (out) {
        const int lane = threadIdx.x & 63, lead = __ffsll((long long)leaving) - 1;
        int base = 0;
        if (lane == lead) base = atomicAdd(&cursor[trash], __popcll(leaving));
        base = __shfl(base, lead, 64);
        perm[base + __popcll(leaving & ((1ull << lane) - 1ull))] = (int)t;
        return;
    }
    perm[atomicAdd(&cursor[c], 1)] = (int)t;
}
// the slots inside a cell were handed out in order of arrival: order every cell's slice by the previous index, which makes the
// sort stable and its result independent of the scheduling.  cnt: the residents of every cell when its slice holds room for new tracers
// behind them (NULL: the slice is the residents)
__global__ __launch_bounds__(256) void k_m3_cell_order(int m, const int* __restrict__ start, const int* __restrict__ cnt, int* __restrict__ perm) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= m) return;
    int* a = perm + start[c];
    const int k = cnt ? cnt[c] : start[c + 1] - start[c];
    if (k <= 32) {
        for (int i = 1; i < k; i++) { const int v = a[i]; int j = i - 1; while (j >= 0 && a[j] > v) { a[j + 1] = a[j]; j--; } a[j + 1] = v; }
        return;
    }
    for (int top = k / 2 - 1, end = k; end > 1;) {            // heap sort: a crowded cell must not cost k^2
        int root, v;
        if (top >= 0) { root = top; v = a[top]; top--; }
        else { end--; v = a[end]; a[end] = a[0]; root = 0; }
        for (;;) {
            int ch = 2 * root + 1;
            if (ch >= end) break;
            if (ch + 1 < end && a[ch + 1] > a[ch]) ch++;
            if (a[ch] <= v) break;
            a[root] = a[ch]; root = ch;
        }
        a[root] = v;
    }
}
// dst[j * dstride + p] = g(src[perm[p] * ts + j * cs]) for ncol columns; bit j of logmask: g = log (geometric averaging);
// perm[p] < 0: the slot of a tracer that k_m3_inject writes
__global__ __launch_bounds__(256) void k_m3_take(long long n, const double* __restrict__ src, long long ts, long long cs, int ncol,
                                                 const int* __restrict__ perm, double* __restrict__ dst, long long dstride, unsigned logmask) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const long long t = perm ? (long long)perm[p] : p;
    if (t < 0) return;
    for (int j = 0; j < ncol; j++) {
        const double v = src[t * ts + j * cs];
        dst[j * dstride + p] = ((logmask >> j) & 1u) ? log(v) : v;
    }
}
// SoA -> (n, ncol) host layout
__global__ __launch_bounds__(256) void k_m3_to_aos(long long n, const double* __restrict__ src, long long cs, int ncol, double* __restrict__ dst) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    for (int j = 0; j < ncol; j++) dst[t * ncol + j] = src[j * cs + t];
}
__global__ __launch_bounds__(256) void k_m3_census(int m, const int* __restrict__ start, int* __restrict__ cnt) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < m) cnt[c] = start[c + 1] - start[c];
}


// ---------------------------------------------------------------------------------------------------------------------
// refill of depleted cells (the extension of pylamp2.py:588-633 by one axis), fused into the sort
// ---------------------------------------------------------------------------------------------------------------------
// block partials of the largest tracer ID (NaN ignored); with key, over the survivors of this sort only (key == trash: the tracer leaves)
__global__ __launch_bounds__(256) void k_m3_max(long long n, const double* __restrict__ x, const int* __restrict__ key, int trash, double* __restrict__ part) {
    double m[1] = {-INFINITY};
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256)
        if (!key || key[t] != trash) m[0] = fmax(m[0], x[t]);
    r3_block<R3All<R3_MAX, 1>>(m, threadIdx.x, blockIdx.x, part);
}
// The new tracers of the deficient cells, written into the room the sort left behind the residents of each cell.  One wave per
// deficient cell, taken from the compacted list (in a typical step a few cells in a million are deficient: a thread per cell would
// idle 63 lanes of 64 and touch 64 cache lines with every load).  Lane j < 13 sums column j of the residents one after the other in
// resident order -- a fixed order, no atomics, so two runs agree bitwise; then lane q writes the q-th new tracer, column by column
// (neighbouring lanes, neighbouring addresses).  0 residents: 0/0 = NaN in every field, as in the reference.
//
// INFLOW (pl3_mic_set_inflow: some wall of the context has a material; the rule is in include/pylamp_hip.h): a cell on a wall with
// a material whose own face carries an inward flow hands the wall's plane values, in the wall's columns, to those of its new tracers
// that lie nearer the wall than every resident.  The wall test depends on the cell alone, so it is the same in all 64 lanes; dmin is
// an fmin over the residents (strided: a cell can hold more than 64) with a butterfly; every lane then works on its own tracers q,
// q + 64, ...: the position once, from it the inflow flag, and the value of a column is a select between the mean and the plane's
// entry.  The inflow tracers are counted with ONE add per wave (ballot and popcount), like the trash bucket of k_m3_key.
struct M3Inflow { unsigned mask[6]; const double* mat[6]; Pl3WallFlow fl; int* count; };
struct M3Inject {
    int nref; const int* list; const int* loff; const int* start; const int* cnt; int dens;
    M3Grid g; double* x; double* f; double* v; long long cap;
    unsigned long long seed; unsigned it3; double id0; int unique;
    M3Inflow in;                                                      // read by k_m3_inject<true> only
};
template <bool INFLOW>
__global__ __launch_bounds__(256) void k_m3_inject(M3Inject a) {
    const int w = (int)(((long long)blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (w >= a.nref) return;                                          // the whole wave leaves
    const int c = a.list[w], k = a.cnt[c], t0 = a.start[c], t1 = t0 + k, m = a.dens - k, off = a.loff[w];
    const int ncx = a.g.a[1].n - 1, ncy = a.g.a[2].n - 1;
    const int ic[3] = {c / (ncy * ncx), (c / ncy) % ncx, c % ncy};
    double mean = 0.0;
    if (lane < M3_NFTRAC && lane != M3_ID) {
        const double* col = a.f + (long long)lane * a.cap;
        double s = 0.0;
        for (int t = t0; t < t1; t++) s += col[t];
        mean = s / (double)k;
    }
    if constexpr (INFLOW) {
        // the first wall in the order z0, x0, y0, zL, xL, yL that has a material, touches the cell and flows inward at the cell's face
        int ws = -1, face = 0;
#pragma unroll
        for (int q = 0; q < 6; q++) {
            const int ax = q % 3, p = ax == 0 ? 1 : 0, r = ax == 2 ? 1 : 2;
            const bool here = a.in.mask[q] != 0u && ((a.in.fl.mask >> q) & 1) && ic[ax] == (q < 3 ? 0 : a.g.a[ax].n - 2);
            if (ws < 0 && here) {
                const int fi = ic[p] * (a.g.a[r].n - 1) + ic[r];
                const double un = a.in.fl.un[q][fi];
                if (q < 3 ? un > 0.0 : un < 0.0) { ws = q; face = fi; }
            }
        }
        const int wa = ws < 0 ? 0 : ws % 3;
        const bool low = ws < 3;
        const double wc = low ? a.g.a[wa].c0 : a.g.a[wa].cl;          // the wall's coordinate: c[0] or c[n - 1]
        double dmin = INFINITY;                                       // distance of the nearest resident from the wall (fmin drops a NaN)
        if (ws >= 0) {
            const double* xa = a.x + (long long)wa * a.cap;
            for (int t = t0 + lane; t < t1; t += 64) dmin = fmin(dmin, low ? xa[t] - wc : wc - xa[t]);
            for (int o = 32; o > 0; o >>= 1) dmin = fmin(dmin, __shfl_xor(dmin, o, 64));
        }
        const unsigned cols = ws < 0 ? 0u : a.in.mask[ws];
        const long long nface = ws < 0 ? 0 : (long long)(a.g.a[wa == 0 ? 1 : 0].n - 1) * (a.g.a[wa == 2 ? 1 : 2].n - 1);
        double mj[M3_NFTRAC], pj[M3_NFTRAC];                          // per column: the mean, and what an inflow tracer takes instead
        int rank = 0;
#pragma unroll
        for (int j = 0; j < M3_NFTRAC; j++) {
            mj[j] = __shfl(mean, j, 64);
            pj[j] = mj[j];
            if (j != M3_ID && ((cols >> j) & 1u)) { pj[j] = a.in.mat[ws][(long long)rank * nface + face]; rank++; }
        }
        int ninflow = 0;
        for (int q0 = 0; q0 < m; q0 += 64) {                          // every lane enters every round: the ballot sees the whole wave
            const int q = q0 + lane;
            bool infl = false;
            if (q < m) {
                const long long ord = a.unique ? (long long)off + q + 1 : (long long)off + q - w;
                double xq[3];
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const double g0 = a.g.a[d].c[ic[d]], h = a.g.a[d].c[ic[d] + 1] - g0;
                    const double u = inj_uniform(a.seed, (unsigned)c, (unsigned)q, a.it3 + d);
                    xq[d] = __dadd_rn(g0, __dmul_rn(u, h));           // the expression of the plain kernel: the same bits
                    a.x[(long long)d * a.cap + t1 + q] = xq[d];
                    a.v[(long long)d * a.cap + t1 + q] = 0.0;
                }
                const double xw = wa == 0 ? xq[0] : (wa == 1 ? xq[1] : xq[2]);
                infl = ws >= 0 && (low ? xw - wc : wc - xw) < dmin;
#pragma unroll
                for (int j = 0; j < M3_NFTRAC; j++)
                    a.f[(long long)j * a.cap + t1 + q] = j == M3_ID ? a.id0 + (double)ord : (infl ? pj[j] : mj[j]);
            }
            ninflow += __popcll(__ballot(infl));
        }
        if (lane == 0 && ninflow > 0) atomicAdd(a.in.count, ninflow);
        return;
    }
    for (int j = 0; j < M3_NFTRAC; j++) {
        const double mj = __shfl(mean, j, 64);
        if (j == M3_ID) continue;
        for (int q = lane; q < m; q += 64) a.f[(long long)j * a.cap + t1 + q] = mj;
    }
    for (int q = lane; q < m; q += 64) {
        // pylamp2.py:621-622: numbering starts AT the largest ID and the first new ID of every cell repeats the last one handed out
        const long long ord = a.unique ? (long long)off + q + 1 : (long long)off + q - w;
        a.f[(long long)M3_ID * a.cap + t1 + q] = a.id0 + (double)ord;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const double g0 = a.g.a[d].c[ic[d]], h = a.g.a[d].c[ic[d] + 1] - g0;
            const double u = inj_uniform(a.seed, (unsigned)c, (unsigned)q, a.it3 + d);
            a.x[(long long)d * a.cap + t1 + q] = __dadd_rn(g0, __dmul_rn(u, h));       // the compiler makes one FMA of it: within an ulp of NumPy's two roundings
            a.v[(long long)d * a.cap + t1 + q] = 0.0;                                  // not advected yet
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// tracer -> grid
// ---------------------------------------------------------------------------------------------------------------------
struct M3Scatter {
    const double* x[3];                  // cell-sorted positions
    int nf; const double* val[M3_MAXF]; int scheme[M3_MAXF];     // values in the form that is summed (logarithm taken for GEOMETRIC)
    M3Grid t;                            // target node set
    int ncs[3];                          // sort cells per axis
    const int* lo[3]; const int* hi[3];  // per target node and axis: the range of sort cells that can hold a contributing tracer
    const int* start;
    double* out[M3_MAXF];
};

// One thread per target node; lanes run along y, so neighbouring lanes read neighbouring cells' slices of the sorted arrays.
// NF > 0: field count known at compile time (accumulators stay in registers); 0: generic.
// SEARCH: the thread keeps c(i-1), c(i), c(i+1) of its own node per axis (extended by the end spacing at the ends); a tracer in
// [c(i-1), c(i)) gives the node t = (p - c(i-1)) / (c(i) - c(i-1)), one in [c(i), c(i+1)) gives 1 - t with t = (p - c(i)) / (c(i+1) - c(i)):
// two interval tests per axis, no search, no floor, and one division only for the tracers that contribute.
template <int NF, bool SEARCH>
__global__ __launch_bounds__(256) void k_m3_scatter(M3Scatter a) {
    const int nz = a.t.a[0].n, nx = a.t.a[1].n, ny = a.t.a[2].n;
    const long long node = (long long)blockIdx.x * 256 + threadIdx.x;
    if (node >= (long long)nz * nx * ny) return;
    const int nf = NF > 0 ? NF : a.nf;
    const int k = (int)(node % ny), j = (int)((node / ny) % nx), i = (int)(node / ((long long)ny * nx));
    const int idx[3] = {i, j, k};
    double wsum = 0.0, cnt = 0.0, acc[NF > 0 ? NF : M3_MAXF];
    for (int q = 0; q < nf; q++) acc[q] = 0.0;
    double cm[3], cc[3], cp[3];
    if constexpr (SEARCH) {
#pragma unroll
        for (int d = 0; d < 3; d++) { cm[d] = m3_coord(a.t.a[d], idx[d] - 1); cc[d] = a.t.a[d].c[idx[d]]; cp[d] = m3_coord(a.t.a[d], idx[d] + 1); }
    }
    const int lo2 = a.lo[2][k], hi2 = a.hi[2][k];
    for (int cz = a.lo[0][i]; cz <= a.hi[0][i]; cz++)
        for (int cx = a.lo[1][j]; cx <= a.hi[1][j]; cx++) {
            const long long row = ((long long)cz * a.ncs[1] + cx) * a.ncs[2];
            const int t0 = a.start[row + lo2], t1 = a.start[row + hi2 + 1];        // the cells of a y-row are contiguous
            for (int t = t0; t < t1; t++) {
                double w = 1.0; bool mine = true;
                if constexpr (SEARCH) {
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        const double p = a.x[d][t];
                        if (p >= cm[d] && p < cc[d]) w *= (p - cm[d]) / (cc[d] - cm[d]);
                        else if (p >= cc[d] && p < cp[d]) w *= 1.0 - (p - cc[d]) / (cp[d] - cc[d]);
                        else { mine = false; break; }
                    }
                } else
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const M3Axis& ax = a.t.a[d];
                    const double p = a.x[d][t];
                    double f = m3_cellf(ax, p);
                    f = fmin(fmax(f, -4.0), (double)ax.n + 2.0);
                    const int ie = (int)f, dn = idx[d] - ie;             // the tracer's corners along this axis are ie, ie + 1
                    if (dn != 0 && dn != 1) { mine = false; break; }
                    const double c0 = m3_coord(ax, ie), c1 = m3_coord(ax, ie + 1), tt = (p - c0) / (c1 - c0);
                    w *= dn ? tt : 1.0 - tt;
                }
                if (!mine) continue;
                wsum += w; cnt += 1.0;
                for (int q = 0; q < nf; q++) { const double v = a.val[q][t]; acc[q] += (a.scheme[q] & PL_AVG_WEIGHTED) ? v * w : v; }
            }
        }
    for (int q = 0; q < nf; q++) {
        const double den = (a.scheme[q] & PL_AVG_WEIGHTED) ? wsum : cnt;
        double s = acc[q], r;
        if (a.scheme[q] & PL_AVG_ARITHMETIC) r = s / den;                // nothing received: 0/0 = NaN, as in 2-D
        else { if (isinf(s)) s = 0.0; r = exp(s / den); }                // pylamp_trac.py:301
        a.out[q][node] = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// grid -> tracer, RK4
// ---------------------------------------------------------------------------------------------------------------------
struct M3Loc { int ie[3]; double t[3], h[3], d0[3], d1[3]; bool bad; long long o; };

template <bool SEARCH>
__device__ inline M3Loc m3_locate(const M3Grid& g, const double p[3]) {
    M3Loc c; c.bad = false;
    double f[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        if constexpr (SEARCH) c.bad = c.bad || !(p[d] >= g.a[d].c0 && p[d] < g.a[d].cl);       // outside on any axis, or NaN
        else { f[d] = m3_cellf(g.a[d], p[d]); c.bad = c.bad || !(f[d] >= 0.0 && f[d] <= (double)(g.a[d].n - 2)); }
    }
#pragma unroll
    for (int d = 0; d < 3; d++) {
        int ie; double lo, hi;
        if constexpr (SEARCH) {
            if (c.bad) { ie = 0; lo = g.a[d].c[0]; hi = g.a[d].c[1]; }
            else ie = m3_search_cell(g.a[d], p[d], lo, hi);
        } else { ie = c.bad ? 0 : (int)f[d]; lo = g.a[d].c[ie]; hi = g.a[d].c[ie + 1]; }
        c.ie[d] = ie; c.d0[d] = p[d] - lo; c.d1[d] = hi - p[d]; c.h[d] = hi - lo;
        c.t[d] = c.d0[d] / (c.d0[d] + c.d1[d]);                          // pylamp_trac.py:89-90
    }
    c.o = ((long long)c.ie[0] * g.a[1].n + c.ie[1]) * g.a[2].n + c.ie[2];
    return c;
}
// the eight corners of a cell, corner index (di 2 + dj) 2 + dk
__device__ inline void m3_corners(const double* __restrict__ F, const M3Grid& g, const M3Loc& c, double v[8]) {
    const long long sy = g.a[2].n, sx = (long long)g.a[1].n * sy;
#pragma unroll
    for (int q = 0; q < 8; q++) v[q] = F[c.o + (q >> 2) * sx + ((q >> 1) & 1) * sy + (q & 1)];
}
__device__ inline double m3_trilinear(const double v[8], const double t[3]) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 8; q++) s += ((q >> 2) ? t[0] : 1 - t[0]) * (((q >> 1) & 1) ? t[1] : 1 - t[1]) * ((q & 1) ? t[2] : 1 - t[2]) * v[q];
    return s;
}
// delta_d delta_e F on the faces f = 0 and f = 1 of the cell, interpolated along f at s  (D, E, F: corner-index bits of the axes)
template <int D, int E, int Fb>
__device__ inline double m3_mixed(const double v[8], double s) {
    const double f0 = v[0] - v[E] - v[D] + v[D + E], f1 = v[Fb] - v[E + Fb] - v[D + Fb] + v[D + E + Fb];
    return (1 - s) * f0 + s * f1;
}
// Divergence-conserving interpolation in 3-D: trilinear plus t_d (1 - t_d) (h_d / 2) [M_de / h_e + M_df / h_f],
// the symmetric extension of pylamp_trac.py:98-154.  Out of grid: all three components = defval.
template <bool SEARCH>
__device__ inline void m3_veldiv(const M3Grid& g, const double* __restrict__ Vz, const double* __restrict__ Vx, const double* __restrict__ Vy,
                                 const double p[3], double defval, double u[3], bool& bad) {
    const M3Loc c = m3_locate<SEARCH>(g, p);
    double vz[8], vx[8], vy[8];
    m3_corners(Vz, g, c, vz); m3_corners(Vx, g, c, vx); m3_corners(Vy, g, c, vy);
    const double* t = c.t; const double* h = c.h;
    // corner-index bits: z = 4, x = 2, y = 1
    const double Gz = 0.5 * h[0] * (m3_mixed<4, 2, 1>(vx, 0.25 + 0.5 * t[2]) / h[1] + m3_mixed<4, 1, 2>(vy, 0.25 + 0.5 * t[1]) / h[2]);
    const double Gx = 0.5 * h[1] * (m3_mixed<2, 4, 1>(vz, 0.25 + 0.5 * t[2]) / h[0] + m3_mixed<2, 1, 4>(vy, 0.25 + 0.5 * t[0]) / h[2]);
    const double Gy = 0.5 * h[2] * (m3_mixed<1, 4, 2>(vz, 0.25 + 0.5 * t[1]) / h[0] + m3_mixed<1, 2, 4>(vx, 0.25 + 0.5 * t[0]) / h[1]);
    u[0] = m3_trilinear(vz, t) + t[0] * (1 - t[0]) * Gz;
    u[1] = m3_trilinear(vx, t) + t[1] * (1 - t[1]) * Gx;
    u[2] = m3_trilinear(vy, t) + t[2] * (1 - t[2]) * Gy;
    if (c.bad) { u[0] = defval; u[1] = defval; u[2] = defval; }
    bad = c.bad;
}

struct M3Gather {
    long long n; M3Pos p; M3Grid g;
    int nf; const double* f[M3_MAXF]; double* out[M3_MAXF]; long long os;     // out[k][t * os]
    int method; double defval; int accumulate;                               // LINEAR only: out += value
    unsigned long long* nout;
};
template <bool SEARCH>
__global__ __launch_bounds__(256) void k_m3_gather(M3Gather a) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    const double p[3] = {a.p.x[0][t * a.p.xs], a.p.x[1][t * a.p.xs], a.p.x[2][t * a.p.xs]};
    bool bad;
    if (a.method & PL_INTERP_NEAREST) {
        const M3Loc c = m3_locate<SEARCH>(a.g, p);
        int m = 0; double dm = 0.0;
#pragma unroll
        for (int q = 0; q < 8; q++) {       // exactly rounded products and sums in a fixed order: ties break as np.argmin does
            const double dz = (q >> 2) ? c.d1[0] : c.d0[0], dx = ((q >> 1) & 1) ? c.d1[1] : c.d0[1], dy = (q & 1) ? c.d1[2] : c.d0[2];
            const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dz, dz), __dmul_rn(dx, dx)), __dmul_rn(dy, dy));
            if (q == 0 || d2 < dm) { m = q; dm = d2; }
        }
        const long long sy = a.g.a[2].n, sx = (long long)a.g.a[1].n * sy, o = c.o + (m >> 2) * sx + ((m >> 1) & 1) * sy + (m & 1);
        for (int k = 0; k < a.nf; k++) a.out[k][t * a.os] = c.bad ? a.defval : a.f[k][o];
        bad = c.bad;
    } else if (a.method & PL_INTERP_LINEAR) {
        const M3Loc c = m3_locate<SEARCH>(a.g, p);
        for (int k = 0; k < a.nf; k++) {
            double v[8];
            m3_corners(a.f[k], a.g, c, v);
            const double r = m3_trilinear(v, c.t);
            a.out[k][t * a.os] = c.bad ? a.defval : (a.accumulate ? a.out[k][t * a.os] + r : r);
        }
        bad = c.bad;
    } else {
        double u[3];
        m3_veldiv<SEARCH>(a.g, a.f[0], a.f[1], a.f[2], p, a.defval, u, bad);
        for (int k = 0; k < 3; k++) a.out[k][t * a.os] = u[k];
    }
    if (bad) atomicAdd(a.nout, 1ull);
}

// RK4 with the reference's weights (1,1,1,1)/6 (pylamp_trac.py:385) and v = (x_new - x)/dt; the four stages of a tracer run in
// registers.  Those weights sum to 4/6, so a uniform field U moves a tracer by 2/3 U dt.  classic != 0 (pl3_mic_set_rk4_classic, opt-in)
// takes the classical weights (1,2,2,1)/6 instead, with which it moves by U dt -- what a flow through the walls needs, where the markers
// must carry the volume that the wall flux brings in.  The default arithmetic is untouched.  72 B/tracer: read the position, write the new one and the velocity; the velocity grid is read through the caches.
struct M3Rk4 {
    long long n; M3Pos p; M3Grid g; const double* V[3]; double dt;
    double* xo[3]; double* vo[3]; long long os;
    int fence; double eps, L[3];                   // pylamp2.py:558-572 per axis
    int classic;
};
template <bool SEARCH>
__global__ __launch_bounds__(256) void k_m3_rk4(M3Rk4 a) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    const double x[3] = {a.p.x[0][t * a.p.xs], a.p.x[1][t * a.p.xs], a.p.x[2][t * a.p.xs]};
    const double dt = a.dt;
    double k1[3], k2[3], k3[3], k4[3], q[3]; bool bad;
    m3_veldiv<SEARCH>(a.g, a.V[0], a.V[1], a.V[2], x, 0.0, k1, bad);
    for (int d = 0; d < 3; d++) q[d] = x[d] + 0.5 * dt * k1[d];
    m3_veldiv<SEARCH>(a.g, a.V[0], a.V[1], a.V[2], q, 0.0, k2, bad);
    for (int d = 0; d < 3; d++) q[d] = x[d] + 0.5 * dt * k2[d];
    m3_veldiv<SEARCH>(a.g, a.V[0], a.V[1], a.V[2], q, 0.0, k3, bad);
    for (int d = 0; d < 3; d++) q[d] = x[d] + dt * k3[d];
    m3_veldiv<SEARCH>(a.g, a.V[0], a.V[1], a.V[2], q, 0.0, k4, bad);
    for (int d = 0; d < 3; d++) {
        double xn;
        if (a.classic) xn = x[d] + (1.0 / 6.0) * dt * (k1[d] + 2.0 * k2[d] + 2.0 * k3[d] + k4[d]);
        else xn = x[d] + (1.0 / 6.0) * dt * (k1[d] + k2[d] + k3[d] + k4[d]);
        a.vo[d][t * a.os] = (xn - x[d]) / dt;
        double xf = xn;
        if (a.fence) { if (xf <= 0.0) xf = a.eps; if (xf >= a.L[d]) xf = a.L[d] - a.eps; }
        a.xo[d][t * a.os] = xf;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// per-tracer properties and subgrid diffusion
// ---------------------------------------------------------------------------------------------------------------------
// pylamp2.py:291-303; f = SoA columns with stride cs
__global__ __launch_bounds__(256) void k_m3_props(long long n, double* __restrict__ f, long long cs, int tdep_rho, int tdep_eta, double tref,
                                                  double etamin, double etamax) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const double T = f[M3_TMP * cs + t], rh0 = f[M3_RH0 * cs + t], et0 = f[M3_ET0 * cs + t];
    f[M3_RHO * cs + t] = tdep_rho ? 1.0 / ((f[M3_ALP * cs + t] * (T - tref) + 1.0) / rh0) : rh0;
    if (tdep_eta) {
        const double ace = f[M3_ACE * cs + t], e = et0 * exp(ace / (M3_GASR * T) - ace / (M3_GASR * tref));
        f[M3_ETA * cs + t] = fmin(fmax(e, etamin), etamax);
    } else f[M3_ETA * cs + t] = et0;
}
// pylamp2.py:471-480 with the third axis in the time scale: T holds T_old + dT; Tsub and dTs = Tsub - T are written
__global__ __launch_bounds__(256) void k_m3_subgrid(long long n, const double* __restrict__ f, long long cs, const double* __restrict__ Told,
                                                    double inv2, double dt, double* __restrict__ Tsub, double* __restrict__ dTs) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const double Tn = f[M3_TMP * cs + t], To = Told[t];
    const double dt0 = f[M3_HCP * cs + t] * f[M3_RHO * cs + t] / (f[M3_HCD * cs + t] * inv2);
    const double ts = To - (To - Tn) * exp(-0.5 * dt / dt0);
    Tsub[t] = ts; dTs[t] = ts - Tn;
}
__global__ __launch_bounds__(256) void k_m3_sub(long long n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ o) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n) o[t] = a[t] - b[t];
}

// =====================================================================================================================
// host side
// =====================================================================================================================
struct Mic3 {
    std::map<std::string, void*> bufs; std::map<std::string, size_t> bytes;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // resident tracers: SoA columns of `cap` doubles, cell-sorted on the context's node grid
    long long n = 0, cap = 0; bool have = false;
    double *x = nullptr, *f = nullptr, *v = nullptr;
    double ms[4] = {0, 0, 0, 0};         // device time of the last resident scatter / temperature gather / RK4 / sort
    // largest TR__ID of the resident tracers: reduced on the device when a refill first needs it after an upload, then kept up to
    // date by the refill.  With deletion on, a sort can remove the holder: a refilling sort then reduces the IDs of its survivors
    // itself, every time, and any other sort that removed something sets have_maxid = false
    bool have_maxid = false; double maxid = 0.0;
    bool rk4_classic = false;                        // pl3_mic_set_rk4_classic: RK4 weights (1,2,2,1)/6 instead of the reference's (1,1,1,1)/6
    bool deletion = false;                           // pl3_mic_set_deletion: every sort of the resident tracers drops those outside the box
    long long removed_last = 0, removed_total = 0;   // by the last sort / since the last upload (pl3_tracers_removed)
    bool have_vgrid = false; M3Grid vgrid;           // the padded centre grid of the resident step: uploaded once per context
    bool search = false;                             // pl3_mic_set_search: cells by per-axis search in every marker kernel of this context
    // pl3_mic_set_inflow: per wall of [z0, x0, y0, zL, xL, yL] the columns an inflow tracer takes from the wall (0: no material) and
    // their planes on the device, in ascending column order (buffers "inflow_w" of bufs)
    unsigned inflow_mask[6] = {0, 0, 0, 0, 0, 0}; double* inflow_dev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    long long inflow_last = 0, inflow_total = 0;     // tracers given a wall's material by the last sort / since the last upload
};
static bool m3_has_inflow(const Mic3* M) { unsigned any = 0; for (int w = 0; w < 6; w++) any |= M->inflow_mask[w]; return any != 0u; }
// a refill riding on a sort: what to do, and what the sort found
struct M3Refill {
    int dens, dmin; unsigned long long seed; int it, unique;
    long long ninj = 0, nref = 0, nempty = 0, mincnt = 0;
    const int *list = nullptr, *loff = nullptr, *cnt = nullptr;
};
#define M3_HIP(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return pl3_fail(ctx, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
#define M3_TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
// every copy between host and device is counted (pl3_transfer_stats)
static inline hipError_t m3_copy(pl3_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
    pl3_count_copy(ctx, bytes);
    return hipMemcpyAsync(dst, src, bytes, kind, stream);
}

void pl3_mic_free(void** slot) {
    Mic3* M = (Mic3*)*slot;
    if (!M) return;
    for (auto& b : M->bufs) (void)hipFree(b.second);
    if (M->ev0) (void)hipEventDestroy(M->ev0);
    if (M->ev1) (void)hipEventDestroy(M->ev1);
    delete M;
    *slot = nullptr;
}
static int m3_open(pl3_ctx* ctx, const char* who, Pl3HostView& v, Mic3** out) {
    M3_TRY(pl3_host_view(ctx, &v));
    if (v.nranks > 1) return pl3_fail(ctx, std::string(who) + ": the 3-D marker-in-cell entry points run on one rank (this context has pl3_set_comm attached)");
    M3_HIP(ctx, hipSetDevice(v.device));
    if (!*v.slot) {
        Mic3* M = new Mic3();
        if (hipEventCreate(&M->ev0) != hipSuccess || hipEventCreate(&M->ev1) != hipSuccess) { delete M; return pl3_fail(ctx, "3-D marker-in-cell: event creation failed"); }
        *v.slot = M;
    }
    *out = (Mic3*)*v.slot;
    return 0;
}
template <typename T>
static int m3_buf(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, const char* name, size_t count, T** out) {
    const size_t need = std::max<size_t>(count, 1) * sizeof(T);
    auto it = M->bufs.find(name);
    if (it == M->bufs.end() || M->bytes[name] < need) {
        if (it != M->bufs.end()) { M3_HIP(ctx, hipStreamSynchronize(v.stream)); (void)hipFree(it->second); M->bufs.erase(it); }
        void* p = nullptr;
        M3_HIP(ctx, hipMalloc(&p, need));
        M->bufs[name] = p; M->bytes[name] = need;
    }
    *out = (T*)M->bufs[name];
    return 0;
}
static inline dim3 m3_blocks(long long n) { return dim3((unsigned)((std::max<long long>(n, 1) + 255) / 256)); }

// The bucket table of one axis for the search: at most M3_MAXBIN equal buckets over [c[0], c[n-1]], two per smallest spacing when
// that fits (the walk from a bucket's entry is then at most one step; beyond the cap it simply gets longer).  A bucket's entry is
// the cell of a point just below everything the device can map to the bucket, so it is never above the cell of a point in it.
#define M3_MAXBIN 4096
static void m3_bins(const double* c, int n, std::vector<int>& tab, double& binv) {
    const double L = c[n - 1] - c[0];
    double hmin = L;
    for (int i = 0; i + 1 < n; i++) hmin = std::min(hmin, c[i + 1] - c[i]);
    const double want = std::ceil(2.0 * L / hmin);
    const int nbin = (int)std::min<double>(M3_MAXBIN, std::max<double>(want, 1.0));
    binv = (double)nbin / L;
    tab.resize((size_t)nbin);
    for (int b = 0; b < nbin; b++) {
        const double e = c[0] + ((double)b / binv) * (1.0 - 1e-15);
        const double lo = std::nextafter(std::nextafter(e, -INFINITY), -INFINITY);
        const int i = (int)(std::upper_bound(c, c + n, lo) - c) - 1;
        tab[(size_t)b] = std::min(std::max(i, 0), n - 2);
    }
}
// a node set given by three host coordinate arrays -> device axes (coordinates in the buffer `name`; with the search switched on
// the bucket tables go beside them, into `name`_bin)
static int m3_grid(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, const char* name, const double* const c[3], const int n[3], M3Grid& g) {
    double* d;
    M3_TRY(m3_buf(ctx, v, M, name, (size_t)n[0] + n[1] + n[2], &d));
    for (int a = 0; a < 3; a++) {
        if (n[a] < 2) return pl3_fail(ctx, "3-D marker-in-cell: a node set needs at least 2 coordinates per axis");
        for (int i = 0; i + 1 < n[a]; i++) if (!(c[a][i + 1] > c[a][i])) return pl3_fail(ctx, "3-D marker-in-cell: coordinates must increase");
        g.a[a].nbin = 0; g.a[a].bin = nullptr; g.a[a].binv = 0.0; g.a[a].cl = c[a][n[a] - 1];
    }
    std::vector<int> tab[3];
    if (M->search) {
        for (int a = 0; a < 3; a++) m3_bins(c[a], n[a], tab[a], g.a[a].binv);
        int* db;
        M3_TRY(m3_buf(ctx, v, M, (std::string(name) + "_bin").c_str(), tab[0].size() + tab[1].size() + tab[2].size(), &db));
        size_t boff = 0;
        for (int a = 0; a < 3; a++) {
            M3_HIP(ctx, m3_copy(ctx, db + boff, tab[a].data(), tab[a].size() * sizeof(int), hipMemcpyHostToDevice, v.stream));
            g.a[a].nbin = (int)tab[a].size(); g.a[a].bin = db + boff;
            boff += tab[a].size();
        }
    }
    size_t off = 0;
    for (int a = 0; a < 3; a++) {
        M3_HIP(ctx, m3_copy(ctx, d + off, c[a], (size_t)n[a] * sizeof(double), hipMemcpyHostToDevice, v.stream));
        g.a[a].n = n[a]; g.a[a].c0 = c[a][0]; g.a[a].L = c[a][n[a] - 1] - c[a][0]; g.a[a].h0 = c[a][1] - c[a][0];
        g.a[a].h1 = c[a][n[a] - 1] - c[a][n[a] - 2]; g.a[a].c = d + off;
        off += n[a];
    }
    M3_HIP(ctx, hipStreamSynchronize(v.stream));          // the host arrays may be temporaries of the caller
    return 0;
}
static long long m3_ncells(const M3Grid& s) { return (long long)(s.a[0].n - 1) * (s.a[1].n - 1) * (s.a[2].n - 1); }

// the three launches of the scan (see k_m3_tile_sums); rf: the scans of a refill ride along and the totals are left in *tot
template <int NS>
static void m3_scan_sums(Pl3HostView& v, int m, const int* cnt, M3Need r, int nb, int* bsum, M3Totals* tot, const double* idpart, int nid) {
    hipLaunchKernelGGL(k_m3_tile_sums<NS>, dim3(nb), dim3(256), 0, v.stream, m, cnt, r, nb, bsum);
    hipLaunchKernelGGL(k_m3_scan_sums<NS>, dim3(1), dim3(1024), 0, v.stream, nb, bsum, tot, idpart, nid);
}
// counting sort by cell of the node set s: perm (sorted slot -> previous index) and start (ncell + 1).  With rf the cells that hold
// fewer than rf->dmin tracers get room for rf->dens - count more behind their residents: start describes the slices WITH the room,
// perm has n + rf->ninj slots (-1 in those of the new tracers) and rf carries the counters and the list of the deficient cells.
// With trash (the resident tracers of a context with deletion on) the tracers outside the box go to a bucket behind the last cell:
// the scans, the census and the refill see the m cells alone, start[m] is the number of tracers that stay (with the room for the new
// ones), the leavers sit in perm[start[m] .. start[m] + *trash) in no particular order and nothing reads them.
static int m3_sort(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, const char* tag, long long n, const M3Pos& p, const M3Grid& s, int** perm_out, int** start_out,
                   M3Refill* rf = nullptr, long long* trash = nullptr) {
    const long long m = m3_ncells(s);
    if (m >= (1ll << 31) - 1 || n >= (1ll << 31) - 1) return pl3_fail(ctx, "3-D marker-in-cell: more than 2^31 cells or tracers");
    int *key, *perm, *cnt, *start, *cur, *bsum; M3Totals* tot;
    const std::string t(tag);
    const int nb = (int)((m + M3_TILE - 1) / M3_TILE), del = trash ? 1 : 0;
    M3_TRY(m3_buf(ctx, v, M, (t + "_key").c_str(), (size_t)n, &key));
    M3_TRY(m3_buf(ctx, v, M, (t + "_cnt").c_str(), (size_t)m + 1, &cnt));
    M3_TRY(m3_buf(ctx, v, M, (t + "_start").c_str(), (size_t)m + 1, &start));
    M3_TRY(m3_buf(ctx, v, M, (t + "_cur").c_str(), (size_t)m + 1, &cur));
    M3_TRY(m3_buf(ctx, v, M, (t + "_bsum").c_str(), (size_t)nb * 5, &bsum));
    M3_TRY(m3_buf(ctx, v, M, (t + "_tot").c_str(), (size_t)1, &tot));
    M3_HIP(ctx, hipMemsetAsync(cnt, 0, (size_t)(m + del) * sizeof(int), v.stream));
    if (n > 0) {
        const dim3 g = m3_blocks(n), b(256);
        if (M->search && del) hipLaunchKernelGGL((k_m3_key<true, true>), g, b, 0, v.stream, n, p, s, key, cnt);
        else if (M->search) hipLaunchKernelGGL((k_m3_key<true, false>), g, b, 0, v.stream, n, p, s, key, cnt);
        else if (del) hipLaunchKernelGGL((k_m3_key<false, true>), g, b, 0, v.stream, n, p, s, key, cnt);
        else hipLaunchKernelGGL((k_m3_key<false, false>), g, b, 0, v.stream, n, p, s, key, cnt);
    }
    int hcnt = 0;                                     // the trash count: a small read-back that only a context with deletion on makes
    long long slots = n;
    if (!rf) {
        const M3Need none{0, 0};
        M3_TRY(m3_buf(ctx, v, M, (t + "_perm").c_str(), (size_t)n, &perm));
        m3_scan_sums<1>(v, (int)m, cnt, none, nb, bsum, tot, nullptr, 0);
        hipLaunchKernelGGL(k_m3_scan_tiles<1>, dim3(nb), dim3(256), 0, v.stream, (int)m, (const int*)cnt, none, nb, (const int*)bsum, (const M3Totals*)tot,
                           start, cur, (int*)nullptr, (int*)nullptr, del);
        if (del && n > 0) {
            M3_HIP(ctx, hipGetLastError());
            M3_HIP(ctx, m3_copy(ctx, &hcnt, cnt + m, sizeof(int), hipMemcpyDeviceToHost, v.stream));
            M3_HIP(ctx, hipStreamSynchronize(v.stream));
        }
    } else {
        const M3Need need{rf->dens, rf->dmin};
        double* idpart = nullptr; int nid = 0;
        // with deletion on the largest ID is that of THIS sort's survivors: reduced here every time, the cached value is not trusted
        if ((!M->have_maxid || del) && rf->dmin > 0) {
            nid = (int)std::min<long long>(1024, (std::max<long long>(n, 1) + 255) / 256);
            M3_TRY(m3_buf(ctx, v, M, (t + "_idpart").c_str(), (size_t)nid, &idpart));
            hipLaunchKernelGGL(k_m3_max, dim3(nid), dim3(256), 0, v.stream, n, (const double*)(M->f + (long long)M3_ID * M->cap),
                               (const int*)(del ? key : nullptr), (int)m, idpart);
        }
        m3_scan_sums<3>(v, (int)m, cnt, need, nb, bsum, tot, idpart, nid);
        M3_HIP(ctx, hipGetLastError());
        M3Totals h;                                   // the one read-back of a refill: how many tracers the arrays must hold
        M3_HIP(ctx, m3_copy(ctx, &h, tot, sizeof(h), hipMemcpyDeviceToHost, v.stream));
        if (del && n > 0) M3_HIP(ctx, m3_copy(ctx, &hcnt, cnt + m, sizeof(int), hipMemcpyDeviceToHost, v.stream));
        M3_HIP(ctx, hipStreamSynchronize(v.stream));
        rf->ninj = h.v[1]; rf->nref = h.v[2]; rf->nempty = h.v[3]; rf->mincnt = m > 0 ? h.v[4] : 0;
        if (idpart) { M->maxid = std::isfinite(h.maxid) ? h.maxid : -1.0; M->have_maxid = true; }     // no finite ID: numbering starts at 0
        slots = n + rf->ninj;
        if (slots >= (1ll << 31) - 1) return pl3_fail(ctx, "3-D marker-in-cell: the refill would take the tracers beyond 2^31");
        int *list, *loff;
        M3_TRY(m3_buf(ctx, v, M, (t + "_perm").c_str(), (size_t)slots, &perm));
        M3_TRY(m3_buf(ctx, v, M, (t + "_list").c_str(), (size_t)rf->nref, &list));
        M3_TRY(m3_buf(ctx, v, M, (t + "_loff").c_str(), (size_t)rf->nref, &loff));
        if (rf->ninj > 0) M3_HIP(ctx, hipMemsetAsync(perm, 0xff, (size_t)slots * sizeof(int), v.stream));
        hipLaunchKernelGGL(k_m3_scan_tiles<3>, dim3(nb), dim3(256), 0, v.stream, (int)m, (const int*)cnt, need, nb, (const int*)bsum, (const M3Totals*)tot,
                           start, cur, list, loff, del);
        rf->list = list; rf->loff = loff; rf->cnt = cnt;
    }
    if (trash) *trash = hcnt;
    if (n > 0) {
        if (del) hipLaunchKernelGGL(k_m3_place_del, m3_blocks(n), dim3(256), 0, v.stream, n, (const int*)key, cur, perm, (int)m);
        else hipLaunchKernelGGL(k_m3_place, m3_blocks(n), dim3(256), 0, v.stream, n, (const int*)key, cur, perm);
        hipLaunchKernelGGL(k_m3_cell_order, m3_blocks(m), dim3(256), 0, v.stream, (int)m, (const int*)start, (const int*)(slots > n ? cnt : nullptr), perm);
    }
    M3_HIP(ctx, hipGetLastError());
    *perm_out = perm; *start_out = start;
    return 0;
}

// tracer -> grid on cell-sorted device tracers: tc = host coordinates of the target node set, sc = of the node set whose cells the
// tracers are sorted by (sort == target: pass the same arrays); out[k] device arrays of the target size
static int m3_scatter_device(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, M3Scatter& a, const double* const tc[3], const int tn[3],
                             const double* const sc[3], const int sn[3], const int* start) {
    if (a.nf < 1 || a.nf > M3_MAXF) return pl3_fail(ctx, "trac2grid (3-D): 1..8 fields per call");
    for (int k = 0; k < a.nf; k++)
        if (!(a.scheme[k] & (PL_AVG_ARITHMETIC | PL_AVG_GEOMETRIC))) return pl3_fail(ctx, "!!! ERROR INVALID AVERAGING SCHEME");
    M3_TRY(m3_grid(ctx, v, M, "sc_tgrid", tc, tn, a.t));
    // sort cells that can hold a tracer with target node i among its corners: the node's support reaches from its lower to its upper
    // neighbour (extended by one spacing at the ends; everything beyond sits in the end cells of the sort, which are clamped)
    std::vector<int> tab((size_t)2 * (tn[0] + tn[1] + tn[2]));
    size_t off = 0; int* d_tab;
    M3_TRY(m3_buf(ctx, v, M, "sc_ranges", tab.size(), &d_tab));
    for (int d = 0; d < 3; d++) {
        const int n = tn[d], ns = sn[d], nc = ns - 1;
        a.ncs[d] = nc;
        const bool same = n == ns && tc[d][0] == sc[d][0] && tc[d][n - 1] == sc[d][ns - 1];
        const double s0 = sc[d][0], Ls = sc[d][ns - 1] - sc[d][0];
        for (int i = 0; i < n; i++) {
            int lo, hi;
            if (same) { lo = i - 1; hi = i; }                      // the tracer's cell and the sort cell come from the same expression
            else if (M->search) {
                // the sort cells of the ends of the node's support [c(i-1), c(i+1)), found as the kernels find them; one more cell on
                // either side where an end coincides with a sort coordinate
                const double pl = i > 0 ? tc[d][i - 1] : tc[d][0] - (tc[d][1] - tc[d][0]);
                const double ph = i < n - 1 ? tc[d][i + 1] : tc[d][n - 1] + (tc[d][n - 1] - tc[d][n - 2]);
                const double* ul = std::upper_bound(sc[d], sc[d] + ns, pl); const double* uh = std::upper_bound(sc[d], sc[d] + ns, ph);
                lo = (int)(ul - sc[d]) - 1; hi = (int)(uh - sc[d]) - 1;
                if (ul != sc[d] && ul[-1] == pl) lo--;
                if (uh != sc[d] && uh[-1] == ph) hi++;
            } else {
                const double pl = i > 0 ? tc[d][i - 1] : tc[d][0] - (tc[d][1] - tc[d][0]);
                const double ph = i < n - 1 ? tc[d][i + 1] : tc[d][n - 1] + (tc[d][n - 1] - tc[d][n - 2]);
                lo = (int)std::floor(std::min(std::max((ns - 1) * (pl - s0) / Ls - 1e-6, -1.0), (double)ns));
                hi = (int)std::floor(std::min(std::max((ns - 1) * (ph - s0) / Ls + 1e-6, -1.0), (double)ns));
            }
            tab[off + i] = std::min(std::max(lo, 0), nc - 1);
            tab[off + n + i] = std::min(std::max(hi, 0), nc - 1);
        }
        a.lo[d] = d_tab + off; a.hi[d] = d_tab + off + n;
        off += 2 * (size_t)n;
    }
    M3_HIP(ctx, m3_copy(ctx, d_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, v.stream));
    M3_HIP(ctx, hipStreamSynchronize(v.stream));
    a.start = start;
    const long long N = (long long)tn[0] * tn[1] * tn[2];
    if (M->search) {
        if (a.nf == 1) hipLaunchKernelGGL((k_m3_scatter<1, true>), m3_blocks(N), dim3(256), 0, v.stream, a);
        else if (a.nf == 2) hipLaunchKernelGGL((k_m3_scatter<2, true>), m3_blocks(N), dim3(256), 0, v.stream, a);
        else if (a.nf == 6) hipLaunchKernelGGL((k_m3_scatter<6, true>), m3_blocks(N), dim3(256), 0, v.stream, a);
        else hipLaunchKernelGGL((k_m3_scatter<0, true>), m3_blocks(N), dim3(256), 0, v.stream, a);
    } else if (a.nf == 1) hipLaunchKernelGGL((k_m3_scatter<1, false>), m3_blocks(N), dim3(256), 0, v.stream, a);
    else if (a.nf == 2) hipLaunchKernelGGL((k_m3_scatter<2, false>), m3_blocks(N), dim3(256), 0, v.stream, a);
    else if (a.nf == 6) hipLaunchKernelGGL((k_m3_scatter<6, false>), m3_blocks(N), dim3(256), 0, v.stream, a);
    else hipLaunchKernelGGL((k_m3_scatter<0, false>), m3_blocks(N), dim3(256), 0, v.stream, a);
    M3_HIP(ctx, hipGetLastError());
    return 0;
}

// the host picks the instantiation: with the switch off the kernels are the regular-grid code
static void m3_launch_gather(Pl3HostView& v, Mic3* M, const M3Gather& a) {
    if (M->search) hipLaunchKernelGGL(k_m3_gather<true>, m3_blocks(a.n), dim3(256), 0, v.stream, a);
    else hipLaunchKernelGGL(k_m3_gather<false>, m3_blocks(a.n), dim3(256), 0, v.stream, a);
}
static void m3_launch_rk4(Pl3HostView& v, Mic3* M, const M3Rk4& a) {
    if (M->search) hipLaunchKernelGGL(k_m3_rk4<true>, m3_blocks(a.n), dim3(256), 0, v.stream, a);
    else hipLaunchKernelGGL(k_m3_rk4<false>, m3_blocks(a.n), dim3(256), 0, v.stream, a);
}

static unsigned m3_logmask(int nf, const int* scheme) {
    unsigned m = 0;
    for (int k = 0; k < nf; k++) if ((scheme[k] & PL_AVG_GEOMETRIC) && !(scheme[k] & PL_AVG_ARITHMETIC)) m |= 1u << k;
    return m;
}

// ---- host-array entry points ----------------------------------------------------------------------------------------
extern "C" int pl3_trac2grid(pl3_ctx* ctx, int64_t n, const double* tr_x, const double* tr_f, int64_t ld_f, int nf, const int* avgscheme,
                             const double* zc, int nzc, const double* xc, int nxc, const double* yc, int nyc, double* const* out) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_trac2grid", v, &M));
    if (n < 0 || (n > 0 && (!tr_x || !tr_f)) || !avgscheme || !zc || !xc || !yc || !out || ld_f < nf) return pl3_fail(ctx, "pl3_trac2grid: bad argument");
    if (nf < 1 || nf > M3_MAXF) return pl3_fail(ctx, "pl3_trac2grid: 1..8 fields per call");
    const double* tc[3] = {zc, xc, yc}; const int tn[3] = {nzc, nxc, nyc};
    const size_t N = (size_t)nzc * nxc * nyc, nn = (size_t)std::max<int64_t>(n, 1);
    double *aos, *xs, *vals, *dout;
    M3_TRY(m3_buf(ctx, v, M, "h_aos", nn * (size_t)(3 + ld_f), &aos));
    M3_TRY(m3_buf(ctx, v, M, "h_x", nn * 3, &xs));
    M3_TRY(m3_buf(ctx, v, M, "h_val", nn * (size_t)nf, &vals));
    M3_TRY(m3_buf(ctx, v, M, "h_out", N * (size_t)nf, &dout));
    M3Grid sg;
    M3_TRY(m3_grid(ctx, v, M, "h_sgrid", tc, tn, sg));
    if (n > 0) {
        M3_HIP(ctx, m3_copy(ctx, aos, tr_x, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, v.stream));
        M3_HIP(ctx, m3_copy(ctx, aos + 3 * nn, tr_f, (size_t)n * ld_f * sizeof(double), hipMemcpyHostToDevice, v.stream));
    }
    M3Pos p{{aos, aos + 1, aos + 2}, 3};
    int *perm, *start;
    M3_TRY(m3_sort(ctx, v, M, "h", n, p, sg, &perm, &start));
    if (n > 0) {
        hipLaunchKernelGGL(k_m3_take, m3_blocks(n), dim3(256), 0, v.stream, (long long)n, (const double*)aos, 3ll, 1ll, 3, (const int*)perm, xs, (long long)nn, 0u);
        hipLaunchKernelGGL(k_m3_take, m3_blocks(n), dim3(256), 0, v.stream, (long long)n, (const double*)(aos + 3 * nn), (long long)ld_f, 1ll, nf,
                           (const int*)perm, vals, (long long)nn, m3_logmask(nf, avgscheme));
    }
    M3Scatter a{};
    for (int d = 0; d < 3; d++) a.x[d] = xs + d * nn;
    a.nf = nf;
    for (int k = 0; k < nf; k++) { a.val[k] = vals + k * nn; a.scheme[k] = avgscheme[k]; a.out[k] = dout + k * N; }
    M3_TRY(m3_scatter_device(ctx, v, M, a, tc, tn, tc, tn, start));
    for (int k = 0; k < nf; k++) M3_HIP(ctx, m3_copy(ctx, out[k], dout + k * N, N * sizeof(double), hipMemcpyDeviceToHost, v.stream));
    M3_HIP(ctx, hipStreamSynchronize(v.stream));
    return 0;
}

static int m3_fields_up(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, const char* name, int nf, const double* const* fields, size_t GN, double** d) {
    M3_TRY(m3_buf(ctx, v, M, name, GN * (size_t)nf, d));
    for (int k = 0; k < nf; k++) M3_HIP(ctx, m3_copy(ctx, *d + k * GN, fields[k], GN * sizeof(double), hipMemcpyHostToDevice, v.stream));
    return 0;
}

extern "C" int pl3_grid2trac(pl3_ctx* ctx, int64_t n, const double* tr_x, int nf, const double* const* fields, int gnz, int gnx, int gny,
                             const double* gz, const double* gx, const double* gy, int method, double defval, int stop_on_error, double* out,
                             int64_t ld_out, int64_t* n_outside) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_grid2trac", v, &M));
    if (n < 0 || (n > 0 && (!tr_x || !out)) || !fields || !gz || !gx || !gy || ld_out < nf) return pl3_fail(ctx, "pl3_grid2trac: bad argument");
    if (nf < 1 || nf > M3_MAXF) return pl3_fail(ctx, "pl3_grid2trac: 1..8 fields per call");
    if (!(method & (PL_INTERP_LINEAR | PL_INTERP_NEAREST | PL_INTERP_VELDIV))) return pl3_fail(ctx, "pl3_grid2trac: unknown interpolation method");
    if (!(method & (PL_INTERP_LINEAR | PL_INTERP_NEAREST)) && nf != 3) return pl3_fail(ctx, "grid2trac(): method INTERP_METHOD_VELDIV expects the fields (vz, vx, vy)");
    const double* gc[3] = {gz, gx, gy}; const int gn[3] = {gnz, gnx, gny};
    const size_t GN = (size_t)gnz * gnx * gny, nn = (size_t)std::max<int64_t>(n, 1);
    double *dx, *df, *dout; unsigned long long* cnt;
    M3_TRY(m3_buf(ctx, v, M, "h_aos", nn * 3, &dx));
    M3_TRY(m3_buf(ctx, v, M, "h_gout", nn * (size_t)nf, &dout));
    M3_TRY(m3_buf(ctx, v, M, "h_counter", (size_t)8, &cnt));
    M3_HIP(ctx, hipMemsetAsync(cnt, 0, sizeof(*cnt), v.stream));
    M3Gather a{};
    M3_TRY(m3_grid(ctx, v, M, "h_ggrid", gc, gn, a.g));
    M3_TRY(m3_fields_up(ctx, v, M, "h_gfields", nf, fields, GN, &df));
    if (n > 0) M3_HIP(ctx, m3_copy(ctx, dx, tr_x, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, v.stream));
    a.n = n; a.p = M3Pos{{dx, dx + 1, dx + 2}, 3}; a.nf = nf; a.os = nf; a.method = method; a.defval = defval; a.accumulate = 0; a.nout = cnt;
    for (int k = 0; k < nf; k++) { a.f[k] = df + k * GN; a.out[k] = dout + k; }
    if (n > 0) m3_launch_gather(v, M, a);
    M3_HIP(ctx, hipGetLastError());
    unsigned long long nout = 0;
    M3_HIP(ctx, m3_copy(ctx, &nout, cnt, sizeof(nout), hipMemcpyDeviceToHost, v.stream));
    M3_HIP(ctx, hipStreamSynchronize(v.stream));
    if (n_outside) *n_outside = (int64_t)nout;
    if (stop_on_error && nout > 0) return pl3_fail(ctx, "stopOnError in grid2trac");
    if (n > 0) {
        pl3_count_copy(ctx, (size_t)n * nf * sizeof(double));
        M3_HIP(ctx, hipMemcpy2DAsync(out, (size_t)ld_out * sizeof(double), dout, (size_t)nf * sizeof(double), (size_t)nf * sizeof(double), (size_t)n,
                                     hipMemcpyDeviceToHost, v.stream));
        M3_HIP(ctx, hipStreamSynchronize(v.stream));
    }
    return 0;
}

extern "C" int pl3_rk4(pl3_ctx* ctx, int64_t n, const double* tr_x, int gnz, int gnx, int gny, const double* gz, const double* gx, const double* gy,
                       const double* vz, const double* vx, const double* vy, double tstep, double* v_out, double* x_out) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_rk4", v, &M));
    if (n < 0 || (n > 0 && (!tr_x || !v_out || !x_out)) || !gz || !gx || !gy || !vz || !vx || !vy) return pl3_fail(ctx, "pl3_rk4: bad argument");
    const double* gc[3] = {gz, gx, gy}; const int gn[3] = {gnz, gnx, gny}; const double* vel[3] = {vz, vx, vy};
    const size_t GN = (size_t)gnz * gnx * gny, nn = (size_t)std::max<int64_t>(n, 1);
    double *dx, *df;
    M3_TRY(m3_buf(ctx, v, M, "h_aos", nn * 9, &dx));
    M3Rk4 a{};
    M3_TRY(m3_grid(ctx, v, M, "h_ggrid", gc, gn, a.g));
    M3_TRY(m3_fields_up(ctx, v, M, "h_gfields", 3, vel, GN, &df));
    if (n > 0) M3_HIP(ctx, m3_copy(ctx, dx, tr_x, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, v.stream));
    a.n = n; a.p = M3Pos{{dx, dx + 1, dx + 2}, 3}; a.dt = tstep; a.os = 3; a.fence = 0; a.classic = M->rk4_classic ? 1 : 0;
    for (int d = 0; d < 3; d++) { a.V[d] = df + d * GN; a.xo[d] = dx + 3 * nn + d; a.vo[d] = dx + 6 * nn + d; }
    if (n > 0) {
        m3_launch_rk4(v, M, a);
        M3_HIP(ctx, hipGetLastError());
        M3_HIP(ctx, m3_copy(ctx, x_out, dx + 3 * nn, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, v.stream));
        M3_HIP(ctx, m3_copy(ctx, v_out, dx + 6 * nn, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, v.stream));
    }
    M3_HIP(ctx, hipStreamSynchronize(v.stream));
    return 0;
}

// ---- resident tracers -----------------------------------------------------------------------------------------------
static int m3_node_grid(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, M3Grid& g) { return m3_grid(ctx, v, M, "r_ngrid", v.coord, v.gn, g); }
static int m3_need_tracers(pl3_ctx* ctx, Mic3* M, const char* who) {
    return M->have ? 0 : pl3_fail(ctx, std::string(who) + ": no resident tracers (pl3_tracers_upload first)");
}
// (re-)sort the resident columns x | f | v by cell into the other of two buffers, which then becomes the resident one.  rf: refill
// the depleted cells in the same pass; when the arrays outgrow `cap`, the other buffer is simply allocated with a larger column
// stride (k_m3_take has separate strides for source and destination), with an eighth of headroom so that a run that injects a
// little in every step does not reallocate in every step.  Every other buffer sized by cap follows at its next use (m3_buf).
static int m3_resort(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, M3Refill* rf = nullptr) {
    M3Grid sg;
    M3_TRY(m3_node_grid(ctx, v, M, sg));
    const long long n = M->n, cap = M->cap;
    M3_HIP(ctx, hipEventRecord(M->ev0, v.stream));
    M3Pos p{{M->x, M->x + cap, M->x + 2 * cap}, 1};
    int *perm, *start;
    long long removed = 0;
    M3_TRY(m3_sort(ctx, v, M, "r", n, p, sg, &perm, &start, rf, M->deletion ? &removed : nullptr));
    M->removed_last = removed; M->removed_total += removed;
    if (removed > 0 && !(rf && rf->dmin > 0)) M->have_maxid = false;      // the holder of the cached largest ID may be among them
    const long long nn = n - removed + (rf ? rf->ninj : 0);               // = start[ncell]: the take below leaves the trash bucket behind
    const long long ncap = nn <= cap ? cap : ((nn + nn / 8 + 63) / 64) * 64;
    double* alt;
    M3_TRY(m3_buf(ctx, v, M, M->x == (double*)M->bufs["r_a"] ? "r_b" : "r_a", (size_t)ncap * (6 + M3_NFTRAC), &alt));
    if (n > 0) {
        hipLaunchKernelGGL(k_m3_take, m3_blocks(nn), dim3(256), 0, v.stream, nn, (const double*)M->x, 1ll, cap, 3, (const int*)perm, alt, ncap, 0u);
        hipLaunchKernelGGL(k_m3_take, m3_blocks(nn), dim3(256), 0, v.stream, nn, (const double*)M->f, 1ll, cap, M3_NFTRAC, (const int*)perm, alt + 3 * ncap, ncap, 0u);
        hipLaunchKernelGGL(k_m3_take, m3_blocks(nn), dim3(256), 0, v.stream, nn, (const double*)M->v, 1ll, cap, 3, (const int*)perm, alt + (3 + M3_NFTRAC) * ncap, ncap, 0u);
    }
    M->x = alt; M->f = alt + 3 * ncap; M->v = alt + (3 + M3_NFTRAC) * ncap; M->n = nn; M->cap = ncap;
    M->inflow_last = 0;
    int hinflow = 0; const int* counted = nullptr;    // the inflow count: a small read-back that only a context with a material makes
    if (rf && rf->nref > 0) {
        M3Inject a{};
        a.nref = (int)rf->nref; a.list = rf->list; a.loff = rf->loff; a.start = start; a.cnt = rf->cnt; a.dens = rf->dens;
        a.g = sg; a.x = M->x; a.f = M->f; a.v = M->v; a.cap = ncap;
        a.seed = rf->seed; a.it3 = 3u * (unsigned)rf->it; a.id0 = M->maxid; a.unique = rf->unique;
        if (m3_has_inflow(M)) {
            // the flow planes are those of the context at this moment (pl3_stokes_set_wall_flow may have replaced them since the last sort)
            int* dcount;
            M3_TRY(m3_buf(ctx, v, M, "inflow_count", (size_t)1, &dcount));
            M3_HIP(ctx, hipMemsetAsync(dcount, 0, sizeof(int), v.stream));
            for (int w = 0; w < 6; w++) { a.in.mask[w] = M->inflow_mask[w]; a.in.mat[w] = M->inflow_dev[w]; }
            a.in.fl = v.wallflow; a.in.count = dcount;
            hipLaunchKernelGGL(k_m3_inject<true>, m3_blocks(rf->nref * 64), dim3(256), 0, v.stream, a);
            counted = dcount;
        } else
            hipLaunchKernelGGL(k_m3_inject<false>, m3_blocks(rf->nref * 64), dim3(256), 0, v.stream, a);
        M->maxid += (double)(rf->unique ? rf->ninj : rf->ninj - rf->nref);
    }
    M3_HIP(ctx, hipGetLastError());
    M3_HIP(ctx, hipEventRecord(M->ev1, v.stream));
    if (counted) M3_HIP(ctx, m3_copy(ctx, &hinflow, counted, sizeof(int), hipMemcpyDeviceToHost, v.stream));
    M3_HIP(ctx, hipStreamSynchronize(v.stream));
    M->inflow_last = hinflow; M->inflow_total += hinflow;
    float ms = 0; (void)hipEventElapsedTime(&ms, M->ev0, M->ev1); M->ms[3] = ms;
    return 0;
}

// The switch is context state: it selects the kernel instantiations of every marker call of this context.  The resident tracers are
// "sorted by cell", so a change re-sorts them by the new rule; the cached padded velocity grid is rebuilt with (or without) its tables.
extern "C" int pl3_mic_set_search(pl3_ctx* ctx, int on) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_mic_set_search", v, &M));
    const bool s = on != 0;
    if (s == M->search) return 0;
    M->search = s; M->have_vgrid = false;
    return M->have ? m3_resort(ctx, v, M) : 0;
}
extern "C" int pl3_mic_get_search(pl3_ctx* ctx, int* on) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_mic_get_search", v, &M));
    if (!on) return pl3_fail(ctx, "pl3_mic_get_search: NULL argument");
    *on = M->search ? 1 : 0;
    return 0;
}

// Deletion is context state like the search: every sort of the resident tracers of this context then drops the tracers outside the
// box.  Switching it on re-sorts resident tracers, which removes those that are outside already; switching it off changes no state.
extern "C" int pl3_mic_set_deletion(pl3_ctx* ctx, int on) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_mic_set_deletion", v, &M));
    const bool d = on != 0;
    if (d == M->deletion) return 0;
    M->deletion = d;
    return d && M->have ? m3_resort(ctx, v, M) : 0;
}
extern "C" int pl3_mic_get_deletion(pl3_ctx* ctx, int* on) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_mic_get_deletion", v, &M));
    if (!on) return pl3_fail(ctx, "pl3_mic_get_deletion: NULL argument");
    *on = M->deletion ? 1 : 0;
    return 0;
}
// The RK4 weights are context state like the search and the deletion: read by pl3_rk4, pl3_resident_rk4 / _advect and pl3_resident_step.
extern "C" int pl3_mic_set_rk4_classic(pl3_ctx* ctx, int on) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_mic_set_rk4_classic", v, &M));
    M->rk4_classic = on != 0;
    return 0;
}
extern "C" int pl3_mic_get_rk4_classic(pl3_ctx* ctx, int* on) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_mic_get_rk4_classic", v, &M));
    if (!on) return pl3_fail(ctx, "pl3_mic_get_rk4_classic: NULL argument");
    *on = M->rk4_classic ? 1 : 0;
    return 0;
}
extern "C" int pl3_tracers_removed(pl3_ctx* ctx, int64_t out[2]) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_tracers_removed", v, &M));
    if (!out) return pl3_fail(ctx, "pl3_tracers_removed: NULL argument");
    out[0] = M->removed_last; out[1] = M->removed_total;
    return 0;
}

// The inflow material is context state like the search, the deletion and the RK4 weights: read by every refilling sort, which takes the
// flow planes from the context at that moment.  Setting it touches no resident tracer.
extern "C" int pl3_mic_set_inflow(pl3_ctx* ctx, int wall, unsigned columns, const double* values) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_mic_set_inflow", v, &M));
    if (wall < 0 || wall > 5) return pl3_fail(ctx, "pl3_mic_set_inflow: wall " + std::to_string(wall) + " is not one of 0 ... 5 (z0, x0, y0, zL, xL, yL)");
    const std::string wn = walls3_names[wall];
    if (columns >> M3_ID) {
        int bit = M3_ID;
        while (!((columns >> bit) & 1u)) bit++;
        if (bit == M3_ID) return pl3_fail(ctx, "pl3_mic_set_inflow: the column mask of wall " + wn + " has bit 12 set: TR__ID is handed out by the refill and cannot be prescribed");
        return pl3_fail(ctx, "pl3_mic_set_inflow: the column mask of wall " + wn + " has bit " + std::to_string(bit) + " set: the tracer columns are 0 ... 11");
    }
    if (columns == 0u) { M->inflow_mask[wall] = 0u; return 0; }
    if (!values) return pl3_fail(ctx, "pl3_mic_set_inflow: wall " + wn + " names columns but values is NULL");
    const size_t nface = walls3_count(v.gn, wall, false);
    const int ncol = __builtin_popcount(columns);
    for (int j = 0, r = 0; j < M3_ID; j++) {
        if (!((columns >> j) & 1u)) continue;
        for (size_t i = 0; i < nface; i++)
            if (!std::isfinite(values[(size_t)r * nface + i])) {
                char num[40];
                snprintf(num, sizeof(num), "%g", values[(size_t)r * nface + i]);
                return pl3_fail(ctx, "pl3_mic_set_inflow: wall " + wn + ", column " + std::to_string(j) + " has a non-finite value at index " + std::to_string(i) + " = " + num);
            }
        r++;
    }
    double* d;
    M3_TRY(m3_buf(ctx, v, M, (std::string("inflow_w") + std::to_string(wall)).c_str(), (size_t)ncol * nface, &d));
    M3_HIP(ctx, hipStreamSynchronize(v.stream));          // (nothing of this context is in flight between calls; the copy below is blocking anyway)
    M3_HIP(ctx, m3_copy(ctx, d, values, (size_t)ncol * nface * sizeof(double), hipMemcpyHostToDevice, v.stream));
    M3_HIP(ctx, hipStreamSynchronize(v.stream));          // the host array may be a temporary of the caller
    M->inflow_dev[wall] = d; M->inflow_mask[wall] = columns;
    return 0;
}
extern "C" int pl3_mic_get_inflow(pl3_ctx* ctx, int wall, unsigned* columns, double* values) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_mic_get_inflow", v, &M));
    if (wall < 0 || wall > 5) return pl3_fail(ctx, "pl3_mic_get_inflow: wall " + std::to_string(wall) + " is not one of 0 ... 5 (z0, x0, y0, zL, xL, yL)");
    if (columns) *columns = M->inflow_mask[wall];
    if (!values || !M->inflow_mask[wall]) return 0;
    const size_t count = (size_t)__builtin_popcount(M->inflow_mask[wall]) * walls3_count(v.gn, wall, false);
    M3_HIP(ctx, m3_copy(ctx, values, M->inflow_dev[wall], count * sizeof(double), hipMemcpyDeviceToHost, v.stream));
    M3_HIP(ctx, hipStreamSynchronize(v.stream));
    return 0;
}
extern "C" int pl3_mic_inflow_count(pl3_ctx* ctx, int64_t out[2]) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_mic_inflow_count", v, &M));
    if (!out) return pl3_fail(ctx, "pl3_mic_inflow_count: NULL argument");
    out[0] = M->inflow_last; out[1] = M->inflow_total;
    return 0;
}

extern "C" int pl3_tracers_upload(pl3_ctx* ctx, int64_t n, const double* tr_x, const double* tr_f) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_tracers_upload", v, &M));
    if (n < 0 || (n > 0 && (!tr_x || !tr_f))) return pl3_fail(ctx, "pl3_tracers_upload: bad argument");
    const long long cap = ((std::max<long long>(n, 1) + 63) / 64) * 64;
    double *aos, *a;
    M3_TRY(m3_buf(ctx, v, M, "h_aos", (size_t)cap * (3 + M3_NFTRAC), &aos));
    M3_TRY(m3_buf(ctx, v, M, "r_a", (size_t)cap * (6 + M3_NFTRAC), &a));
    M->n = n; M->cap = cap; M->x = a; M->f = a + 3 * cap; M->v = a + (3 + M3_NFTRAC) * cap; M->have = true; M->have_maxid = false;
    M->removed_last = 0; M->removed_total = 0; M->inflow_last = 0; M->inflow_total = 0;
    M3_HIP(ctx, hipMemsetAsync(a, 0, (size_t)cap * (6 + M3_NFTRAC) * sizeof(double), v.stream));
    if (n > 0) {
        M3_HIP(ctx, m3_copy(ctx, aos, tr_x, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, v.stream));
        M3_HIP(ctx, m3_copy(ctx, aos + 3 * cap, tr_f, (size_t)n * M3_NFTRAC * sizeof(double), hipMemcpyHostToDevice, v.stream));
        hipLaunchKernelGGL(k_m3_take, m3_blocks(n), dim3(256), 0, v.stream, (long long)n, (const double*)aos, 3ll, 1ll, 3, (const int*)nullptr, M->x, cap, 0u);
        hipLaunchKernelGGL(k_m3_take, m3_blocks(n), dim3(256), 0, v.stream, (long long)n, (const double*)(aos + 3 * cap), (long long)M3_NFTRAC, 1ll, M3_NFTRAC,
                           (const int*)nullptr, M->f, cap, 0u);
        M3_HIP(ctx, hipGetLastError());
    }
    return m3_resort(ctx, v, M);
}

static int m3_down(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, const double* src, int ncol, double* host) {
    double* aos;
    M3_TRY(m3_buf(ctx, v, M, "h_aos", (size_t)M->cap * (3 + M3_NFTRAC), &aos));
    if (M->n > 0) {
        hipLaunchKernelGGL(k_m3_to_aos, m3_blocks(M->n), dim3(256), 0, v.stream, M->n, src, M->cap, ncol, aos);
        M3_HIP(ctx, hipGetLastError());
        M3_HIP(ctx, m3_copy(ctx, host, aos, (size_t)M->n * ncol * sizeof(double), hipMemcpyDeviceToHost, v.stream));
    }
    M3_HIP(ctx, hipStreamSynchronize(v.stream));
    return 0;
}
extern "C" int pl3_tracers_download(pl3_ctx* ctx, int64_t n, double* tr_x, double* tr_f) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_tracers_download", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_tracers_download"));
    if (n != M->n || (n > 0 && (!tr_x || !tr_f))) return pl3_fail(ctx, "pl3_tracers_download: n does not match pl3_tracers_count");
    M3_TRY(m3_down(ctx, v, M, M->x, 3, tr_x));
    return m3_down(ctx, v, M, M->f, M3_NFTRAC, tr_f);
}
extern "C" int pl3_tracers_count(pl3_ctx* ctx, int64_t* n) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_tracers_count", v, &M));
    if (!n) return pl3_fail(ctx, "pl3_tracers_count: NULL argument");
    *n = M->have ? M->n : 0;
    return 0;
}
extern "C" int pl3_tracers_census(pl3_ctx* ctx, int64_t ncell, int32_t* counts) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_tracers_census", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_tracers_census"));
    const long long m = (long long)(v.gn[0] - 1) * (v.gn[1] - 1) * (v.gn[2] - 1);
    if (ncell != m || !counts) return pl3_fail(ctx, "pl3_tracers_census: counts must hold (nz-1)(nx-1)(ny-1) cells");
    int* d;
    M3_TRY(m3_buf(ctx, v, M, "r_census", (size_t)m, &d));
    hipLaunchKernelGGL(k_m3_census, m3_blocks(m), dim3(256), 0, v.stream, (int)m, (const int*)M->bufs["r_start"], d);
    M3_HIP(ctx, hipGetLastError());
    M3_HIP(ctx, m3_copy(ctx, counts, d, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, v.stream));
    M3_HIP(ctx, hipStreamSynchronize(v.stream));
    return 0;
}
extern "C" int pl3_get_tracer_velocity(pl3_ctx* ctx, int64_t n, double* out) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_get_tracer_velocity", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_get_tracer_velocity"));
    if (n != M->n || (n > 0 && !out)) return pl3_fail(ctx, "pl3_get_tracer_velocity: n does not match pl3_tracers_count");
    return m3_down(ctx, v, M, M->v, 3, out);
}
extern "C" int pl3_resident_times(pl3_ctx* ctx, double ms[4]) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_resident_times", v, &M));
    for (int k = 0; k < 4; k++) ms[k] = M->ms[k];
    return 0;
}

extern "C" int pl3_resident_props(pl3_ctx* ctx, int tdep_rho, int tdep_eta, double tref, double etamin, double etamax) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_resident_props", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_resident_props"));
    if (M->n > 0) hipLaunchKernelGGL(k_m3_props, m3_blocks(M->n), dim3(256), 0, v.stream, M->n, M->f, M->cap, tdep_rho, tdep_eta, tref, etamin, etamax);
    M3_HIP(ctx, hipGetLastError());
    M3_HIP(ctx, hipStreamSynchronize(v.stream));
    return 0;
}

// scatter of resident columns (val: device pointers, logarithms taken here) to a node set; dout: device (nf x N)
static int m3_resident_scatter(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, int nf, const double* const* col, const int* scheme, const double* const tc[3],
                               const int tn[3], double* dout) {
    const size_t N = (size_t)tn[0] * tn[1] * tn[2];
    M3Scatter a{};
    double* lg;
    M3_TRY(m3_buf(ctx, v, M, "r_log", (size_t)M->cap * M3_MAXF, &lg));
    for (int d = 0; d < 3; d++) a.x[d] = M->x + d * M->cap;
    a.nf = nf;
    for (int k = 0; k < nf; k++) {
        a.scheme[k] = scheme[k]; a.out[k] = dout + k * N; a.val[k] = col[k];
        if (m3_logmask(1, scheme + k) && M->n > 0) {
            hipLaunchKernelGGL(k_m3_take, m3_blocks(M->n), dim3(256), 0, v.stream, M->n, col[k], 1ll, 0ll, 1, (const int*)nullptr, lg + k * M->cap, M->cap, 1u);
            a.val[k] = lg + k * M->cap;
        }
    }
    return m3_scatter_device(ctx, v, M, a, tc, tn, v.coord, v.gn, (const int*)M->bufs["r_start"]);
}

// resident columns -> a node set, into the plain device array dout (nf x N); the device time goes to pl3_resident_times
static int m3_columns_scatter(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, const char* who, int nf, const int* columns, const int* avgscheme,
                              const double* const tc[3], const int tn[3], double* dout) {
    const double* col[M3_MAXF];
    for (int k = 0; k < nf; k++) {
        if (columns[k] < 0 || columns[k] >= M3_NFTRAC) return pl3_fail(ctx, std::string(who) + ": tracer column out of range");
        col[k] = M->f + (long long)columns[k] * M->cap;
    }
    M3_HIP(ctx, hipEventRecord(M->ev0, v.stream));
    M3_TRY(m3_resident_scatter(ctx, v, M, nf, col, avgscheme, tc, tn, dout));
    M3_HIP(ctx, hipEventRecord(M->ev1, v.stream));
    return 0;
}
static int m3_scatter_time(pl3_ctx* ctx, Pl3HostView& v, Mic3* M) {
    M3_HIP(ctx, hipStreamSynchronize(v.stream));
    float ms = 0; (void)hipEventElapsedTime(&ms, M->ev0, M->ev1); M->ms[0] = ms;
    return 0;
}
extern "C" int pl3_resident_trac2grid(pl3_ctx* ctx, int nf, const int* columns, const int* avgscheme, const double* zc, int nzc, const double* xc,
                                      int nxc, const double* yc, int nyc, double* const* out) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_resident_trac2grid", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_resident_trac2grid"));
    if (nf < 1 || nf > M3_MAXF || !columns || !avgscheme || !zc || !xc || !yc || !out) return pl3_fail(ctx, "pl3_resident_trac2grid: bad argument (1..8 fields per call)");
    const double* tc[3] = {zc, xc, yc}; const int tn[3] = {nzc, nxc, nyc};
    const size_t N = (size_t)nzc * nxc * nyc;
    double* dout;
    M3_TRY(m3_buf(ctx, v, M, "r_out", N * (size_t)nf, &dout));
    M3_TRY(m3_columns_scatter(ctx, v, M, "pl3_resident_trac2grid", nf, columns, avgscheme, tc, tn, dout));
    for (int k = 0; k < nf; k++) M3_HIP(ctx, m3_copy(ctx, out[k], dout + k * N, N * sizeof(double), hipMemcpyDeviceToHost, v.stream));
    return m3_scatter_time(ctx, v, M);
}
int pl3i_mic_scatter(pl3_ctx* ctx, int nf, const int* columns, const int* avgscheme, const double* const tc[3], const int tn[3], double* dout) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_resident_step", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_resident_step"));
    M3_TRY(m3_columns_scatter(ctx, v, M, "pl3_resident_step", nf, columns, avgscheme, tc, tn, dout));
    return m3_scatter_time(ctx, v, M);
}
int pl3i_mic_buf(pl3_ctx* ctx, const char* name, size_t count, double** out) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_resident_step", v, &M));
    return m3_buf(ctx, v, M, name, count, out);
}
int pl3i_mic_columns(pl3_ctx* ctx, double** f, long long* n, long long* cap) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_resident_step", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_resident_step"));
    *f = M->f; *n = M->n; *cap = M->cap;
    return 0;
}
double* pl3i_mic_ms(pl3_ctx* ctx) {
    Pl3HostView v; Mic3* M;
    return m3_open(ctx, "pl3_resident_step", v, &M) ? nullptr : M->ms;
}

// Temperature to the tracers (pylamp2.py:445-480): absolute != 0: T = interpolation of `field` (the first step); else T += interpolation
// (field = T_new - T_old on the nodes) and, with subgrid != 0, the subgrid-diffusion correction with tstep.  A tracer outside the
// grid is an error, as with stopOnError in 2-D.
// field: host array, or with dev a plain device array that is read in place
static int m3_temp_to_tracers(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, int absolute, const double* field, bool dev, int subgrid, double tstep) {
    const long long n = M->n, cap = M->cap;
    const size_t GN = (size_t)v.gn[0] * v.gn[1] * v.gn[2];
    double *df = const_cast<double*>(field), *w, *dnode; unsigned long long* cnt;
    if (!dev) M3_TRY(m3_buf(ctx, v, M, "r_tfield", GN, &df));
    M3_TRY(m3_buf(ctx, v, M, "r_twork", (size_t)cap * 3, &w));
    M3_TRY(m3_buf(ctx, v, M, "r_tnode", GN, &dnode));
    M3_TRY(m3_buf(ctx, v, M, "h_counter", (size_t)8, &cnt));
    M3_HIP(ctx, hipMemsetAsync(cnt, 0, sizeof(*cnt), v.stream));
    if (!dev) M3_HIP(ctx, m3_copy(ctx, df, field, GN * sizeof(double), hipMemcpyHostToDevice, v.stream));
    M3Gather a{};
    M3_TRY(m3_node_grid(ctx, v, M, a.g));
    double* T = M->f + M3_TMP * cap;
    const bool sub = !absolute && subgrid;
    M3_HIP(ctx, hipEventRecord(M->ev0, v.stream));
    if (sub) M3_HIP(ctx, hipMemcpyAsync(w, T, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, v.stream));      // T_old
    a.n = n; a.p = M3Pos{{M->x, M->x + cap, M->x + 2 * cap}, 1}; a.nf = 1; a.os = 1; a.method = PL_INTERP_LINEAR; a.defval = NAN;
    a.accumulate = absolute ? 0 : 1; a.nout = cnt; a.f[0] = df; a.out[0] = T;
    if (n > 0) m3_launch_gather(v, M, a);
    if (sub && n > 0) {
        double inv2 = 0.0;
        for (int d = 0; d < 3; d++) { const double h = (v.coord[d][v.gn[d] - 1] - v.coord[d][0]) / (v.gn[d] - 1); inv2 += (2.0 / h) * (2.0 / h); }
        hipLaunchKernelGGL(k_m3_subgrid, m3_blocks(n), dim3(256), 0, v.stream, n, (const double*)M->f, cap, (const double*)w, inv2, tstep, w + cap, w + 2 * cap);
        const double* col[1] = {w + 2 * cap}; const int sch[1] = {PL_AVG_ARITHMETIC | PL_AVG_WEIGHTED};
        M3_TRY(m3_resident_scatter(ctx, v, M, 1, col, sch, v.coord, v.gn, dnode));
        a.f[0] = dnode; a.out[0] = w; a.accumulate = 0;                       // the correction back on the tracers
        m3_launch_gather(v, M, a);
        hipLaunchKernelGGL(k_m3_sub, m3_blocks(n), dim3(256), 0, v.stream, n, (const double*)(w + cap), (const double*)w, T);
    }
    M3_HIP(ctx, hipGetLastError());
    M3_HIP(ctx, hipEventRecord(M->ev1, v.stream));
    unsigned long long nout = 0;
    M3_HIP(ctx, m3_copy(ctx, &nout, cnt, sizeof(nout), hipMemcpyDeviceToHost, v.stream));
    M3_HIP(ctx, hipStreamSynchronize(v.stream));
    float ms = 0; (void)hipEventElapsedTime(&ms, M->ev0, M->ev1); M->ms[1] = ms;
    if (nout > 0) return pl3_fail(ctx, "stopOnError in grid2trac");
    return 0;
}
extern "C" int pl3_resident_temp_to_tracers(pl3_ctx* ctx, int absolute, const double* field, int subgrid, double tstep) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_resident_temp_to_tracers", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_resident_temp_to_tracers"));
    if (!field) return pl3_fail(ctx, "pl3_resident_temp_to_tracers: NULL field");
    return m3_temp_to_tracers(ctx, v, M, absolute, field, false, subgrid, tstep);
}
int pl3i_mic_temp_to_tracers(pl3_ctx* ctx, int absolute, const double* dfield, int subgrid, double tstep) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_resident_step", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_resident_step"));
    return m3_temp_to_tracers(ctx, v, M, absolute, dfield, true, subgrid, tstep);
}

// what a refill may be asked for; out = the four counters of the header
static int m3_refill_args(pl3_ctx* ctx, const Mic3* M, const char* who, int tracdens, int tracdens_min, int fence, const int64_t* out) {
    const std::string w(who);
    if (!out) return pl3_fail(ctx, w + ": NULL out");
    if (tracdens < 0 || tracdens_min < 0) return pl3_fail(ctx, w + ": tracdens and tracdens_min must not be negative");
    if (tracdens_min > 0 && tracdens < tracdens_min) return pl3_fail(ctx, w + ": tracdens < tracdens_min (a refilled cell would still be deficient)");
    if (tracdens_min > 0 && !fence && !M->deletion)
        return pl3_fail(ctx, w + ": tracer injection needs the fence: without it a tracer outside the box would be counted in the nearest "
                                 "cell, and the deletion that pylamp2.py:574-581 does instead needs pl3_mic_set_deletion on this context");
    return 0;
}
static void m3_refill_out(const M3Refill& rf, int64_t out[4]) { out[0] = rf.ninj; out[1] = rf.nref; out[2] = rf.nempty; out[3] = rf.mincnt; }

// RK4 on the padded centre grid (nz+1, nx+1, ny+1), fence (pylamp2.py:558-572, length = the node grid's extent), re-sort (+ refill)
// g / df: the padded centre grid and the three velocity arrays on it, on the device
static int m3_advect_dev(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, const M3Grid& g, const double* df, double tstep, int fence, M3Refill* rf) {
    const size_t GN = (size_t)(v.gn[0] + 1) * (v.gn[1] + 1) * (v.gn[2] + 1);
    const long long n = M->n, cap = M->cap;
    M3Rk4 a{};
    a.g = g;
    a.n = n; a.p = M3Pos{{M->x, M->x + cap, M->x + 2 * cap}, 1}; a.dt = tstep; a.os = 1; a.fence = fence ? 1 : 0; a.eps = 1.0 / 1024.0;   // EPS of pylamp_const.py
    a.classic = M->rk4_classic ? 1 : 0;
    for (int d = 0; d < 3; d++) { a.V[d] = df + d * GN; a.xo[d] = M->x + d * cap; a.vo[d] = M->v + d * cap; a.L[d] = v.coord[d][v.gn[d] - 1]; }
    M3_HIP(ctx, hipEventRecord(M->ev0, v.stream));
    if (n > 0) m3_launch_rk4(v, M, a);       // in place: a tracer reads its position before it writes
    M3_HIP(ctx, hipGetLastError());
    M3_HIP(ctx, hipEventRecord(M->ev1, v.stream));
    M3_HIP(ctx, hipStreamSynchronize(v.stream));
    float ms = 0; (void)hipEventElapsedTime(&ms, M->ev0, M->ev1); M->ms[2] = ms;
    return m3_resort(ctx, v, M, rf);
}
static int m3_advect(pl3_ctx* ctx, Pl3HostView& v, Mic3* M, const char* who, const double* gz, const double* gx, const double* gy, const double* vz,
                     const double* vx, const double* vy, double tstep, int fence, M3Refill* rf) {
    if (!gz || !gx || !gy || !vz || !vx || !vy) return pl3_fail(ctx, std::string(who) + ": bad argument");
    const double* gc[3] = {gz, gx, gy}; const int gn[3] = {v.gn[0] + 1, v.gn[1] + 1, v.gn[2] + 1}; const double* vel[3] = {vz, vx, vy};
    const size_t GN = (size_t)gn[0] * gn[1] * gn[2];
    double* df;
    M3Grid g;
    M3_TRY(m3_grid(ctx, v, M, "r_vgrid", gc, gn, g));
    M3_TRY(m3_fields_up(ctx, v, M, "r_vfields", 3, vel, GN, &df));
    return m3_advect_dev(ctx, v, M, g, df, tstep, fence, rf);
}
// The step's advection: dV = the three padded velocity arrays on the device.  The padded coordinates (pylamp2.py:92-95 and :491-493:
// midpoints, one extrapolated entry at either end) are computed and uploaded once per context.
int pl3i_mic_advect(pl3_ctx* ctx, const double* dV, double tstep, int tracdens, int tracdens_min, uint64_t seed, int it, int unique_ids, int64_t out[4]) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_resident_step", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_resident_step"));
    M3_TRY(m3_refill_args(ctx, M, "pl3_resident_step", tracdens, tracdens_min, M->deletion ? 0 : 1, out));
    const int gn[3] = {v.gn[0] + 1, v.gn[1] + 1, v.gn[2] + 1};
    if (!M->have_vgrid) {
        std::vector<double> c[3];
        for (int d = 0; d < 3; d++) {
            const int n = v.gn[d]; const double* x = v.coord[d];
            c[d].resize((size_t)n + 1);
            for (int i = 0; i + 1 < n; i++) c[d][i + 1] = (x[i + 1] + x[i]) / 2;
            c[d][n] = c[d][n - 1] + (c[d][n - 1] - c[d][n - 2]);
            c[d][0] = c[d][1] - (c[d][2] - c[d][1]);
        }
        const double* gc[3] = {c[0].data(), c[1].data(), c[2].data()};
        M3_TRY(m3_grid(ctx, v, M, "s_vgrid", gc, gn, M->vgrid));
        M->have_vgrid = true;
    }
    M3Refill rf{tracdens, tracdens_min, seed, it, unique_ids ? 1 : 0};
    M3_TRY(m3_advect_dev(ctx, v, M, M->vgrid, dV, tstep, M->deletion ? 0 : 1, &rf));       // the fence is off exactly when the sort deletes
    m3_refill_out(rf, out);
    return 0;
}
extern "C" int pl3_resident_rk4(pl3_ctx* ctx, const double* gz, const double* gx, const double* gy, const double* vz, const double* vx,
                                const double* vy, double tstep, int fence) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_resident_rk4", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_resident_rk4"));
    return m3_advect(ctx, v, M, "pl3_resident_rk4", gz, gx, gy, vz, vx, vy, tstep, fence, nullptr);
}
extern "C" int pl3_resident_advect(pl3_ctx* ctx, const double* gz, const double* gx, const double* gy, const double* vz, const double* vx,
                                   const double* vy, double tstep, int fence, int tracdens, int tracdens_min, uint64_t seed, int it,
                                   int unique_ids, int64_t out[4]) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_resident_advect", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_resident_advect"));
    M3_TRY(m3_refill_args(ctx, M, "pl3_resident_advect", tracdens, tracdens_min, fence, out));
    M3Refill rf{tracdens, tracdens_min, seed, it, unique_ids ? 1 : 0};
    M3_TRY(m3_advect(ctx, v, M, "pl3_resident_advect", gz, gx, gy, vz, vx, vy, tstep, fence, &rf));
    m3_refill_out(rf, out);
    return 0;
}
extern "C" int pl3_resident_refill(pl3_ctx* ctx, int tracdens, int tracdens_min, uint64_t seed, int it, int unique_ids, int64_t out[4]) {
    Pl3HostView v; Mic3* M;
    M3_TRY(m3_open(ctx, "pl3_resident_refill", v, &M));
    M3_TRY(m3_need_tracers(ctx, M, "pl3_resident_refill"));
    M3_TRY(m3_refill_args(ctx, M, "pl3_resident_refill", tracdens, tracdens_min, 1, out));
    M3Refill rf{tracdens, tracdens_min, seed, it, unique_ids ? 1 : 0};
    M3_TRY(m3_resort(ctx, v, M, &rf));
    m3_refill_out(rf, out);
    return 0;
}
