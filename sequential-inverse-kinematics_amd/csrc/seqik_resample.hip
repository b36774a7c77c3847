// seqik_resample.hip -- PCHIP resampling of joint-angle records: the kernels, argument checks, launch code and the C ABI
// entry points of include/seqik_resample.h (values) and include/seqik_resample_der.h (values and derivatives).
//
// Evaluation.  The output of a chain, [n_out][width] doubles, is one flat run of E = n_out * width elements.  A wavefront
// takes a TILE of 64 * rows consecutive elements and stores it as `rows` contiguous 512-byte lines (a record of 7
// doubles aligns with nothing, the flat index does).  The samples of a tile read a contiguous run of knots:
//   staged   the run (+1 knot in front, +2 behind; in bridge mode out to the valid knots of the first and last stencil)
//            comes into LDS with coalesced loads; every needed derivative is computed once per (knot, column), the two
//            leading coefficients of the cubic once per (interval, column); a sample then costs an interval search, four
//            LDS reads and three multiply-adds (DER: two more for the first derivative, one for the second, from the
//            same four values).
//   direct   when the run does not fit (strong downsampling, long gaps in bridge mode) every lane runs
//            seqik::resample_sample_der on global memory: the host restatement itself.
// Both paths run the functions of seqik_resample.hpp in the same order, so they agree with the host bit for bit.
//
// Neighbour tables (bridge mode), over tiles of F = 64 k knots of one chain (k = 1 unless a chain has more than 65 536
// knots, then as small as keeps a chain at <= 1024 tiles):
//   tile  one wavefront per tile: records come in 64 at a time with coalesced loads, a ballot gives the valid knots, and
//         each lane takes the highest set bit at or below it (prev, walking forward) or the lowest at or above it (next,
//         walking back over the prev entries just written); -1 / n_frames where the tile has none.
//   scan  (more than one tile per chain) one wavefront per chain: the last prev entry of every tile is the tile's last
//         valid knot, the first next entry its first one; an inclusive max-scan / reversed min-scan over these <= 1024
//         values is written back in place.
//   fix   one lane per knot: an unresolved entry takes the scanned entry of the neighbouring tile.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "seqik_resample.hpp"
#include "seqik_runtime.hpp"
#include "../../include/seqik_resample.h"
#include "../../include/seqik_resample_der.h"

namespace {

using seqik::bad_arg;
using seqik::kMaxTiles;  // table tiles per chain (scan: 16 rows of 64 lanes)
using seqik::PchipKnot;
using seqik::ResampleParams;
using seqik::wave_lds_fence;

constexpr int kBlock = 256;       // threads per workgroup: 4 independent wavefronts
constexpr int kWaves = kBlock / 64;
constexpr int kStage = 256;       // doubles per LDS array and wavefront: 256 / width knots
constexpr int kMaxRows = 64;      // 512-byte lines per tile (keeps the width division below exact, see div_w)
constexpr int kDivShift = 17;

struct ResampleArgs {
    const double *y;
    double *out, *d1, *d2;  // d1 / d2: the derivative planes of the DER kernels (any of the three may be null there)
    int32_t *prev, *next;
    ResampleParams p;
    int64_t n_chains, tiles_per_chain, chain_elems;  // chain_elems = n_out * width
    int32_t rows;
    uint32_t magic;  // ceil(2^17 / width)
    int64_t tab_tile, tab_tiles;  // F, tiles per chain of the table kernels
};

// x / width for x < 4200: magic = ceil(2^17 / width) errs by less than width <= 16 parts in 2^17
__device__ __forceinline__ int div_w(int x, uint32_t magic) { return (int)(((uint32_t)x * magic) >> kDivShift); }

__device__ __forceinline__ PchipKnot lds_knot(const double *sy, int32_t k, bool has, int32_t lo, int W, int col, double ots)
{
    PchipKnot r;
    r.has = has;
    r.x = has ? seqik::resample_x(k, ots) : 0.0;
    r.y = has ? sy[(k - lo) * W + col] : 0.0;
    return r;
}

// DER = false: the value alone into a.out (seqik_resample_pchip).  DER = true: the value, first and second derivative
// into those of a.out, a.d1, a.d2 that are not null (seqik_resample_der); the staging is the same work either way.
template <bool BRIDGE, bool DER>
__global__ void __launch_bounds__(kBlock) seqik_resample_kernel(ResampleArgs a)
{
    __shared__ double s_y[kWaves][kStage], s_d[kWaves][kStage], s_c0[kWaves][kStage], s_c1[kWaves][kStage];
    __shared__ int32_t s_a[kWaves][BRIDGE ? kStage : 1], s_b[kWaves][BRIDGE ? kStage : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kWaves + wave;
    if (t >= a.n_chains * a.tiles_per_chain) return;
    const ResampleParams &p = a.p;
    const int W = p.width;
    const int32_t n = p.n_frames;
    const int64_t c = t / a.tiles_per_chain, tt = t % a.tiles_per_chain;
    const int64_t E = a.chain_elems;
    const int64_t e0 = tt * (64 * (int64_t)a.rows);
    const int64_t e1 = e0 + 64 * (int64_t)a.rows < E ? e0 + 64 * (int64_t)a.rows : E;
    const int32_t i_first = (int32_t)(e0 / W), i_last = (int32_t)((e1 - 1) / W);
    const int rem0 = (int)(e0 - (int64_t)i_first * W);
    const double *ych = a.y + c * (int64_t)n * W;
    double *och = DER && !a.out ? nullptr : a.out + c * E;
    const bool st0 = !DER || a.out, st1 = DER && a.d1, st2 = DER && a.d2;
    // what a sample computes: the staged path every order of its kernel, the direct path the orders that are stored
    // (!DER: the compile-time kResampleValue)
    constexpr int kWant = DER ? seqik::kResampleAll : seqik::kResampleValue;
    const int want = (st0 ? seqik::kResampleValue : 0) | (st1 ? seqik::kResampleD1 : 0) | (st2 ? seqik::kResampleD2 : 0);
    const int32_t *prev = BRIDGE ? a.prev + c * (int64_t)n : nullptr;
    const int32_t *next = BRIDGE ? a.next + c * (int64_t)n : nullptr;
    const int32_t j_first = seqik::resample_interval(seqik::resample_x(i_first, p.nts), p.ots, p.inv_ots, n);
    const int32_t j_last = seqik::resample_interval(seqik::resample_x(i_last, p.nts), p.ots, p.inv_ots, n);

    // the knots [lo, hi] that hold every stencil of this tile; jf .. jl: the intervals the coefficient pass covers
    int32_t lo, hi, jf, jl;
    if (BRIDGE) {
        lo = jf = j_first;
        hi = jl = j_last;
        int32_t P, A, B, Q;
        bool tail;
        if (seqik::resample_bridge_stencil(prev, next, j_first, n, P, A, B, Q, tail)) lo = P >= 0 ? P : A;
        if (seqik::resample_bridge_stencil(prev, next, j_last, n, P, A, B, Q, tail)) {
            const int32_t top = Q < n ? Q : B;
            hi = top > hi ? top : hi;
        }
    } else {
        jf = j_first < n - 2 ? j_first : n - 2;
        jl = j_last < n - 2 ? j_last : n - 2;
        lo = jf > 0 ? jf - 1 : 0;
        hi = jl + 2 < n ? jl + 2 : n - 1;
    }
    const int64_t nk = (int64_t)hi - lo + 1;

    if (nk * W <= kStage) {
        double *sy = s_y[wave], *sd = s_d[wave], *sc0 = s_c0[wave], *sc1 = s_c1[wave];
        const int cnt = (int)nk * W;
        const double *src = ych + (int64_t)lo * W;
        for (int e = lane; e < cnt; e += 64) sy[e] = src[e];
        wave_lds_fence();
        // derivatives, once per (knot, column); a knot whose neighbours lie outside [lo, hi] is no end of a needed interval
        for (int e = lane; e < cnt; e += 64) {
            const int kk = div_w(e, a.magic), col = e - kk * W;
            const int32_t g = lo + kk;
            seqik::PchipNeighbours k;
            if (!seqik::resample_neighbours(prev, next, BRIDGE, g, n, k)) continue;
            if ((k.hm1 && k.m1 < lo) || (k.hp1 && k.p1 > hi) || (k.hm2 && k.m2 < lo) || (k.hp2 && k.p2 > hi)) continue;
            const PchipKnot K0 = lds_knot(sy, g, true, lo, W, col, p.ots);
            sd[e] = seqik::pchip_deriv(lds_knot(sy, k.m2, k.hm2, lo, W, col, p.ots),
                                       lds_knot(sy, k.m1, k.hm1, lo, W, col, p.ots), K0,
                                       lds_knot(sy, k.p1, k.hp1, lo, W, col, p.ots),
                                       lds_knot(sy, k.p2, k.hp2, lo, W, col, p.ots));
        }
        wave_lds_fence();
        // the two leading coefficients, once per (interval, column)
        const int ni = (int)(jl - jf + 1) * W;
        for (int e = lane; e < ni; e += 64) {
            const int ii = div_w(e, a.magic), col = e - ii * W;
            const int32_t j = jf + ii;
            int32_t A = j, B = j + 1;
            bool ok = true;
            if (BRIDGE) {
                int32_t P, Q;
                bool tail;
                ok = seqik::resample_bridge_stencil(prev, next, j, n, P, A, B, Q, tail);
                if (col == 0) {
                    s_a[wave][j - lo] = ok ? A : -1;
                    s_b[wave][j - lo] = tail ? ~B : B;
                }
                if (!ok) continue;
            }
            const int la = (A - lo) * W + col, lb = (B - lo) * W + col;
            double c0, c1;
            seqik::pchip_coefs(seqik::resample_x(A, p.ots), sy[la], seqik::resample_x(B, p.ots), sy[lb], sd[la], sd[lb],
                               c0, c1);
            if (!BRIDGE) {
                bool fin = seqik::is_finite(sy[la]) && seqik::is_finite(sy[lb]);
                if (A > 0) fin = fin && seqik::is_finite(sy[la - W]);
                if (B + 1 < n) fin = fin && seqik::is_finite(sy[lb + W]);
                if (!fin) c0 = seqik::resample_nan();
            }
            const int lj = (j - lo) * W + col;
            sc0[lj] = c0;
            sc1[lj] = c1;
        }
        wave_lds_fence();
        for (int r = 0; r < a.rows; ++r) {
            const int el = r * 64 + lane;
            const int64_t e = e0 + el;
            if (e >= e1) break;
            const int x = rem0 + el, q = div_w(x, a.magic), col = x - q * W;
            const double u = seqik::resample_x(i_first + q, p.nts);
            const int32_t j = seqik::resample_interval(u, p.ots, p.inv_ots, n);
            double v[3];
            if (BRIDGE) {
                const int32_t A = s_a[wave][j - lo], bt = s_b[wave][j - lo];
                const bool tail = bt < 0;
                const int32_t B = tail ? ~bt : bt;
                if (A < 0 || !seqik::resample_bridge_ok(u, A, B, tail, p.ots, p.max_gap)) {
                    v[0] = v[1] = v[2] = seqik::resample_nan();
                } else {
                    const int la = (A - lo) * W + col, lb = (B - lo) * W + col, lj = (j - lo) * W + col;
                    const bool on_b = tail && u == seqik::resample_x(B, p.ots);
                    seqik::pchip_cubic_orders(sc0[lj], sc1[lj], sd[la], sy[la], u - seqik::resample_x(A, p.ots), on_b,
                                              on_b ? sy[lb] : 0.0, DER && on_b ? sd[lb] : 0.0, kWant, v);
                }
            } else {
                const int32_t A = j < n - 2 ? j : n - 2;
                const int la = (A - lo) * W + col;
                const bool on_b = j == n - 1 && u == seqik::resample_x(A + 1, p.ots);
                seqik::pchip_cubic_orders(sc0[la], sc1[la], sd[la], sy[la], u - seqik::resample_x(A, p.ots), on_b,
                                          on_b ? sy[la + W] : 0.0, DER && on_b ? sd[la + W] : 0.0, kWant, v);
                // What this branch adds: every order is NaN when the stencil holds a non-finite value, as
                // resample_sample_der decides it.  Off knot B the poisoned c0 says so; on it (the last knot's sample
                // alone) y_B and d_B bypass c0, so the stencil n - 3 .. n - 1 is asked itself (an overflowed c0 must not
                // count as a non-finite value)
                if (on_b) {
                    bool fin = seqik::is_finite(sy[la]) && seqik::is_finite(sy[la + W]);
                    if (A > 0) fin = fin && seqik::is_finite(sy[la - W]);
                    if (!fin) v[0] = v[1] = v[2] = seqik::resample_nan();
                }
            }
            if (st0) __builtin_nontemporal_store(v[0], och + e);
            if (st1) __builtin_nontemporal_store(v[1], a.d1 + c * E + e);
            if (st2) __builtin_nontemporal_store(v[2], a.d2 + c * E + e);
        }
    } else {
        for (int r = 0; r < a.rows; ++r) {
            const int el = r * 64 + lane;
            const int64_t e = e0 + el;
            if (e >= e1) break;
            const int x = rem0 + el, q = div_w(x, a.magic), col = x - q * W;
            double v[3];
            seqik::resample_sample_der(ych, prev, next, p, i_first + q, col, want, v);
            if (st0) och[e] = v[0];
            if (st1) a.d1[c * E + e] = v[1];
            if (st2) a.d2[c * E + e] = v[2];
        }
    }
}

__device__ __forceinline__ void table_tile(const ResampleArgs &a, int64_t wid, int64_t &c, int64_t &f0, int64_t &f1)
{
    c = wid / a.tab_tiles;
    f0 = (wid % a.tab_tiles) * a.tab_tile;
    f1 = f0 + a.tab_tile < a.p.n_frames ? f0 + a.tab_tile : a.p.n_frames;
}

__global__ void __launch_bounds__(kBlock) seqik_resample_tables_tile_kernel(ResampleArgs a)
{
    __shared__ int s_bad[kWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wid = (int64_t)blockIdx.x * kWaves + wave;
    if (wid >= a.n_chains * a.tab_tiles) return;
    int64_t c, f0, f1;
    table_tile(a, wid, c, f0, f1);
    const int W = a.p.width;
    const int32_t n = a.p.n_frames;
    const double *ych = a.y + c * (int64_t)n * W;
    int32_t *prev = a.prev + c * (int64_t)n, *next = a.next + c * (int64_t)n;
    int *bad = s_bad[wave];
    int32_t carry = -1;
    for (int64_t b = f0; b < f1; b += 64) {
        const int nf = (int)(f1 - b < 64 ? f1 - b : 64);
        bad[lane] = 0;
        wave_lds_fence();
        const double *src = ych + b * W;
        for (int e = lane; e < nf * W; e += 64)
            if (!seqik::is_finite(src[e])) bad[div_w(e, a.magic)] = 1;
        wave_lds_fence();
        const bool valid = lane < nf && !bad[lane];
        const uint64_t mask = __ballot(valid);
        const uint64_t le = mask & (lane == 63 ? ~0ull : (2ull << lane) - 1ull);
        if (lane < nf) prev[b + lane] = le ? (int32_t)(b + 63 - __builtin_clzll(le)) : carry;
        if (mask) carry = (int32_t)(b + 63 - __builtin_clzll(mask));
        wave_lds_fence();  // the next block's flags stay behind these reads
    }
    int32_t carry_n = n;
    const int64_t nb = (f1 - f0 + 63) / 64;
    for (int64_t bb = nb - 1; bb >= 0; --bb) {
        const int64_t b = f0 + bb * 64;
        const int nf = (int)(f1 - b < 64 ? f1 - b : 64);
        // each lane reads back the entry it wrote above
        const bool valid = lane < nf && prev[b + lane] == (int32_t)(b + lane);
        const uint64_t mask = __ballot(valid);
        const uint64_t ge = mask & ~((1ull << lane) - 1ull);
        if (lane < nf) next[b + lane] = ge ? (int32_t)(b + __builtin_ctzll(ge)) : carry_n;
        if (mask) carry_n = (int32_t)(b + __builtin_ctzll(mask));
    }
}

// one wavefront per chain: inclusive max-scan of the tiles' last prev entries and, from the right, min-scan of their
// first next entries, in place
__global__ void __launch_bounds__(kBlock) seqik_resample_tables_scan_kernel(ResampleArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * kWaves + wave;
    if (c >= a.n_chains) return;
    const int64_t n = a.p.n_frames, T = a.tab_tiles, F = a.tab_tile;
    int32_t *prev = a.prev + c * n, *next = a.next + c * n;
    int32_t v[kMaxTiles / 64], w[kMaxTiles / 64];
#pragma unroll
    for (int i = 0; i < kMaxTiles / 64; ++i) {
        const int64_t j = (int64_t)i * 64 + lane;
        const int64_t end = (j + 1) * F < n ? (j + 1) * F - 1 : n - 1;
        v[i] = j < T ? prev[end] : -1;
        w[i] = j < T ? next[(T - 1 - j) * F] : (int32_t)n;  // tiles from the right
    }
    int32_t cv = -1, cw = (int32_t)n;
#pragma unroll
    for (int i = 0; i < kMaxTiles / 64; ++i) {
        int32_t x = v[i], z = w[i];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t xo = __shfl_up(x, d, 64), zo = __shfl_up(z, d, 64);
            if (lane >= d) {
                x = xo > x ? xo : x;
                z = zo < z ? zo : z;
            }
        }
        x = cv > x ? cv : x;
        z = cw < z ? cw : z;
        const int64_t j = (int64_t)i * 64 + lane;
        if (j < T) {
            const int64_t end = (j + 1) * F < n ? (j + 1) * F - 1 : n - 1;
            prev[end] = x;
            next[(T - 1 - j) * F] = z;
        }
        cv = __shfl(x, 63, 64);
        cw = __shfl(z, 63, 64);
    }
}

// one lane per knot: what its own tile left open comes from the scanned entry of the neighbouring tile (which this
// kernel never writes: a tile's last prev entry and first next entry are final after the scan)
__global__ void __launch_bounds__(kBlock) seqik_resample_tables_fix_kernel(ResampleArgs a, int64_t blocks_per_chain)
{
    const int64_t c = blockIdx.x / blocks_per_chain;
    const int64_t j = (blockIdx.x % blocks_per_chain) * kBlock + threadIdx.x;
    const int64_t n = a.p.n_frames, F = a.tab_tile;
    if (j >= n) return;
    int32_t *prev = a.prev + c * n, *next = a.next + c * n;
    const int64_t ts = (j / F) * F, te = ts + F < n ? ts + F - 1 : n - 1;
    if (j != te && ts > 0 && prev[j] < 0) prev[j] = prev[ts - 1];
    if (j != ts && te + 1 < n && next[j] >= n) next[j] = next[te + 1];
}

bool step_ok(double ts) { return ts == ts && ts >= 0x1p-500 && ts <= 0x1p500; }

// n_out or a negative error code
int64_t count_checked(const char *who, int64_t n_frames, double ots, double nts)
{
    if (n_frames < 2) return bad_arg(who, "n_frames must be at least 2 (an interpolant needs two knots)");
    if (n_frames > INT32_MAX) return bad_arg(who, "n_frames must be below 2^31");
    if (!step_ok(ots) || !step_ok(nts))
        return bad_arg(who, "original_ts and new_ts must be finite and positive (2^-500 .. 2^500)");
    const double cnt = seqik::resample_count_f64(n_frames, ots, nts);
    if (!(cnt >= 1.0) || cnt > (double)INT32_MAX) return bad_arg(who, "the sample count per chain must lie in 1 .. 2^31 - 1");
    return (int64_t)cnt;
}

// The checks every entry point makes before anything touches HIP.  der: "out" stands for the planes that were asked for.
int resample_validate(const char *who, bool der, const double *y, int64_t n_chains, int64_t n_frames, int32_t width,
                      double ots, double nts, int32_t flags, const double *out, const double *d1, const double *d2,
                      int64_t n_out)
{
    if (der && !out && !d1 && !d2) return bad_arg(who, "out_value, out_d1 and out_d2 are all null: ask for at least one");
    if (der && !out) out = d1 ? d1 : d2;
    if (n_chains < 0) return bad_arg(who, "negative n_chains");
    if (width < 1 || width > seqik::kResampleMaxWidth) return bad_arg(who, "width must lie in 1..16");
    if (flags & ~SEQIK_RESAMPLE_BRIDGE) return bad_arg(who, "unknown flags (0 or SEQIK_RESAMPLE_BRIDGE)");
    const int64_t cnt = count_checked(who, n_frames, ots, nts);
    if (cnt < 0) return (int)cnt;
    if (n_out != cnt) return bad_arg(who, "n_out must be seqik_resample_count(n_frames, original_ts, new_ts)");
    if (!y || !out) return bad_arg(who, "y and out must not be null");
    // the byte count of either array must fit in 63 bits
    const int64_t lim = INT64_MAX / (8 * width);
    if (n_chains != 0 && (n_chains > lim / n_out || n_chains > lim / n_frames)) return bad_arg(who, "too many values");
    return SEQIK_OK;
}

// What the device entry points do: the checks, the tile geometry, then the table kernels (bridge mode) and the evaluation
// kernel on `hip_stream`.  DER = false: d_out alone; DER = true: the planes that are not null.
template <bool DER>
int resample_enqueue(const char *who, const double *d_y, int64_t n_chains, int64_t n_frames, int32_t width,
                     double original_ts, double new_ts, int32_t flags, int32_t max_gap, double *d_out, double *d_d1,
                     double *d_d2, int64_t n_out, void *d_workspace, void *hip_stream)
{
    const int rc = resample_validate(who, DER, d_y, n_chains, n_frames, width, original_ts, new_ts, flags, d_out, d_d1, d_d2,
                                     n_out);
    if (rc != SEQIK_OK) return rc;
    const bool bridge = flags & SEQIK_RESAMPLE_BRIDGE;
    if (bridge && !d_workspace) return bad_arg(who, "bridge mode needs d_workspace (seqik_resample_workspace_bytes)");
    if (n_chains == 0) return SEQIK_OK;
    ResampleArgs a;
    memset(&a, 0, sizeof(a));
    a.y = d_y;
    a.out = d_out;
    a.d1 = d_d1;
    a.d2 = d_d2;
    a.prev = bridge ? static_cast<int32_t *>(d_workspace) : nullptr;
    a.next = bridge ? a.prev + n_chains * n_frames : nullptr;
    a.p = seqik::resample_params(original_ts, new_ts, (int32_t)n_frames, (int32_t)n_out, width, flags, max_gap);
    a.n_chains = n_chains;
    a.chain_elems = n_out * width;
    // as many 512-byte lines per tile as keep the tile's knots (+ 4 for the stencils) within the LDS stage
    const double lines = (double)(kStage / width - 4) * (original_ts / new_ts) * width / 64.0;
    a.rows = lines >= (double)kMaxRows ? kMaxRows : (lines >= 1.0 ? (int32_t)lines : 1);
    a.magic = ((1u << kDivShift) + (uint32_t)width - 1u) / (uint32_t)width;
    a.tiles_per_chain = (a.chain_elems + 64 * (int64_t)a.rows - 1) / (64 * (int64_t)a.rows);
    seqik::tile_geometry(n_frames, &a.tab_tile, &a.tab_tiles);
    const int64_t blocks = seqik::blocks_for(n_chains * a.tiles_per_chain, kWaves);
    const int64_t tab_blocks = seqik::blocks_for(n_chains * a.tab_tiles, kWaves), fix_per_chain = (n_frames + kBlock - 1) / kBlock;
    if (blocks > INT32_MAX || (bridge && (tab_blocks > INT32_MAX || n_chains * fix_per_chain > INT32_MAX)))
        return bad_arg(who, "too many values for one launch");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (bridge) {
        hipLaunchKernelGGL(seqik_resample_tables_tile_kernel, dim3((unsigned)tab_blocks), dim3(kBlock), 0, s, a);
        HIP_TRY(hipGetLastError());
        if (a.tab_tiles > 1) {
            hipLaunchKernelGGL(seqik_resample_tables_scan_kernel, dim3((unsigned)seqik::blocks_for(n_chains, kWaves)), dim3(kBlock), 0, s,
                               a);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(seqik_resample_tables_fix_kernel, dim3((unsigned)(n_chains * fix_per_chain)), dim3(kBlock),
                               0, s, a, fix_per_chain);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL((seqik_resample_kernel<true, DER>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    } else {
        hipLaunchKernelGGL((seqik_resample_kernel<false, DER>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    }
    return seqik::launched();
}

// What the host entry points do: the checks, then one HostCall around resample_enqueue, which reports as `who_device`.
template <bool DER>
int resample_host(const char *who, const char *who_device, const double *y, int64_t n_chains, int64_t n_frames,
                  int32_t width, double original_ts, double new_ts, int32_t flags, int32_t max_gap, double *out,
                  double *out_d1, double *out_d2, int64_t n_out, int32_t device)
{
    int rc = resample_validate(who, DER, y, n_chains, n_frames, width, original_ts, new_ts, flags, out, out_d1, out_d2, n_out);
    if (rc != SEQIK_OK) return rc;
    if (n_chains == 0) return SEQIK_OK;
    const size_t n_rows = (size_t)width * (size_t)n_chains;
    seqik::HostCall call;
    double *d_y, *d_out, *d_d1, *d_d2;
    char *d_ws;
    call.upload(d_y, n_rows * (size_t)n_frames, y);
    call.download(d_out, n_rows * (size_t)n_out, out);
    call.download(d_d1, n_rows * (size_t)n_out, out_d1);
    call.download(d_d2, n_rows * (size_t)n_out, out_d2);
    call.scratch(d_ws, seqik_resample_workspace_bytes(n_chains, n_frames, flags));
    if ((rc = call.begin(device)) != SEQIK_OK) return rc;
    return call.finish(resample_enqueue<DER>(who_device, d_y, n_chains, n_frames, width, original_ts, new_ts, flags, max_gap,
                                             d_out, d_d1, d_d2, n_out, d_ws, call.stream()));
}

}  // namespace

extern "C" {

int64_t seqik_resample_count(int64_t n_frames, double original_ts, double new_ts)
{
    return count_checked("seqik_resample_count", n_frames, original_ts, new_ts);
}

size_t seqik_resample_workspace_bytes(int64_t n_chains, int64_t n_frames, int32_t flags)
{
    if (!(flags & SEQIK_RESAMPLE_BRIDGE) || n_chains <= 0 || n_frames <= 0) return 0;
    return (size_t)n_chains * (size_t)n_frames * 2 * sizeof(int32_t);
}

int seqik_resample_pchip_device(const double *d_y, int64_t n_chains, int64_t n_frames, int32_t width,
                                double original_ts, double new_ts, int32_t flags, int32_t max_gap, double *d_out,
                                int64_t n_out, void *d_workspace, void *hip_stream)
{
    return resample_enqueue<false>("seqik_resample_pchip_device", d_y, n_chains, n_frames, width, original_ts, new_ts, flags,
                                   max_gap, d_out, nullptr, nullptr, n_out, d_workspace, hip_stream);
}

int seqik_resample_pchip(const double *y, int64_t n_chains, int64_t n_frames, int32_t width, double original_ts,
                         double new_ts, int32_t flags, int32_t max_gap, double *out, int64_t n_out, int32_t device)
{
    return resample_host<false>("seqik_resample_pchip", "seqik_resample_pchip_device", y, n_chains, n_frames, width,
                                original_ts, new_ts, flags, max_gap, out, nullptr, nullptr, n_out, device);
}

int seqik_resample_der_device(const double *d_y, int64_t n_chains, int64_t n_frames, int32_t width, double original_ts,
                              double new_ts, int32_t flags, int32_t max_gap, double *d_value, double *d_d1, double *d_d2,
                              int64_t n_out, void *d_workspace, void *hip_stream)
{
    return resample_enqueue<true>("seqik_resample_der_device", d_y, n_chains, n_frames, width, original_ts, new_ts, flags,
                                  max_gap, d_value, d_d1, d_d2, n_out, d_workspace, hip_stream);
}

int seqik_resample_der(const double *y, int64_t n_chains, int64_t n_frames, int32_t width, double original_ts,
                       double new_ts, int32_t flags, int32_t max_gap, double *out_value, double *out_d1, double *out_d2,
                       int64_t n_out, int32_t device)
{
    return resample_host<true>("seqik_resample_der", "seqik_resample_der_device", y, n_chains, n_frames, width, original_ts,
                               new_ts, flags, max_gap, out_value, out_d1, out_d2, n_out, device);
}

}  // extern "C"
