// Rank counts of the classifier's test-set report (gfx950): metrics.recog_auc / recog_pr / recog_acc (metrics.py:9-96) without
// a sort.  The reference hands the N x C score matrix to sklearn's roc_curve / auc / average_precision_score; both numbers
// are rank statistics of the N positive scores p_i = s[i][y[i]], so what the device has to deliver is, for every row i, how
// many elements of a population lie at or above p_i (DESIGN section 6c has the fold):
//   micro      population = all N*C scores,       positives = the N scores p_j
//   per class  population = column y[i],          positives = the rows j with y[j] == y[i]
//   rank_prep_kernel    scores -> order-preserving int keys, transposed to keyT[C][N] with the rows in label-grouped order
//                       (so a column AND the positives of a class are contiguous ranges), p_i, argmax test, input checks
//   rank_count_kernel   all thresholds against all population elements: a lane keeps RK_K thresholds in registers, the
//                       population streams through LDS in tiles that every lane reads at the same address (broadcast),
//                       inner work = integer compare + add-with-carry into int32 counters, combined with integer atomics
//                       (exact, so the result does not depend on the grid or on the order of arrival)
#include "common.h"
#include <limits.h>

namespace {

constexpr int RK_THREADS = 256;                  // 4 waves: one per SIMD
constexpr int RK_K = 4;                          // thresholds per lane
constexpr int RK_TB = RK_THREADS * RK_K;         // thresholds per block
constexpr int RK_TILE = 2048;                    // population elements per LDS tile (8 KiB)
constexpr int RK_LOADS = RK_TILE / RK_THREADS;   // elements a thread stages per tile
constexpr int RK_BLOCKS_PER_CU = 16;             // grid target (measured at 12630 x 43: 4 -> 1.03 ms, 8 -> 0.89, 16 -> 0.87, 24 -> 0.88)

// float -> int whose signed order is the order of the float VALUES: -0.0 and +0.0 get the same key, denormals keep theirs
// (a float compare may flush them; numpy on the host does not)
__device__ __forceinline__ int rank_key(float v) {
  int b = __float_as_int(v);
  if (b == INT_MIN) b = 0;
  return b ^ ((b >> 31) & INT_MAX);
}
__device__ __forceinline__ bool rank_finite(float v) { return (__float_as_int(v) & 0x7f800000) != 0x7f800000; }

// Keys of finite floats lie in [0x80800000, 0x7f7fffff]: INT_MIN as an ELEMENT is below every threshold (counted nowhere: tile
// padding, non-finite scores, rows without a valid label), INT_MAX as a THRESHOLD is above every element (counts nothing: lanes
// without a row, rows of another class).

// One thread per grouped position r (row order[r]; order = the rows sorted by label, made by the caller).
__global__ __launch_bounds__(RK_THREADS) void rank_prep_kernel(const float* __restrict__ scores, const long long* __restrict__ labels,
                                                               const int* __restrict__ order, int N, int C, int* __restrict__ keyT,
                                                               int* __restrict__ posg, int* __restrict__ glab, int* correct, int* err) {
  const int r = blockIdx.x * RK_THREADS + threadIdx.x;
  int bad = 0;
  bool hit = false;
  if (r < N) {
    const int i = order[r];
    if (i < 0 || i >= N) {                       // not a row: nothing of it enters a population
      bad = 1;
      for (int c = 0; c < C; ++c) keyT[(size_t)c * N + r] = INT_MIN;
      posg[r] = INT_MIN;
      glab[r] = -1;
    } else {
      const long long y = labels[i];
      const bool valid = y >= 0 && y < C;
      bad += !valid;
      if (r > 0) {                               // the grouping the count kernel relies on
        const int ip = order[r - 1];
        if (ip >= 0 && ip < N && labels[ip] > y) ++bad;
      }
      const float* row = scores + (size_t)i * C;
      const float pf = valid ? row[y] : 0.f;
      const int p = rank_key(pf);
      hit = valid && rank_finite(pf);
      for (int c = 0; c < C; ++c) {
        const float v = row[c];
        const bool fin = rank_finite(v);
        const int k = fin ? rank_key(v) : INT_MIN;
        bad += !fin;
        keyT[(size_t)c * N + r] = k;
        hit = hit && fin && (c < y ? p > k : p >= k);          // np.argmax: the first maximum wins
      }
      posg[r] = valid && rank_finite(pf) ? p : INT_MIN;
      glab[r] = valid ? (int)y : -1;
    }
  }
  if (bad) atomicAdd(err, bad);
  const unsigned long long m = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(correct, __popcll(m));
}

// ge[k] += #{e in pop[0 .. len): e >= thr[k]}, gt[k] likewise with >.  Block-uniform pop / len (the loop holds barriers).
// The next tile's global loads are issued before the current tile is counted.
__device__ __forceinline__ void rank_stream(const int* __restrict__ pop, int len, const int (&thr)[RK_K], int (&ge)[RK_K], int (&gt)[RK_K],
                                            int* tile) {
  const int t = threadIdx.x;
  if (len <= 0) return;
  int nxt[RK_LOADS];
#pragma unroll
  for (int m = 0; m < RK_LOADS; ++m) { const int idx = m * RK_THREADS + t; nxt[m] = idx < len ? pop[idx] : INT_MIN; }
  for (int base = 0; base < len; base += RK_TILE) {
    __syncthreads();                             // the previous tile (of this or an earlier call) has been read
#pragma unroll
    for (int m = 0; m < RK_LOADS; ++m) tile[m * RK_THREADS + t] = nxt[m];
    __syncthreads();
    if (base + RK_TILE < len) {
#pragma unroll
      for (int m = 0; m < RK_LOADS; ++m) { const int idx = base + RK_TILE + m * RK_THREADS + t; nxt[m] = idx < len ? pop[idx] : INT_MIN; }
    }
    const int rest = len - base;
    const int lim = rest >= RK_TILE ? RK_TILE : (rest + 3) & ~3;          // the padding up to a multiple of 4 is INT_MIN
#pragma unroll 4
    for (int j = 0; j < lim; j += 4) {
      const int4 v = *(const int4*)(tile + j);   // same address in every lane: an LDS broadcast
#pragma unroll
      for (int k = 0; k < RK_K; ++k) {
        ge[k] += (v.x >= thr[k]) + (v.y >= thr[k]) + (v.z >= thr[k]) + (v.w >= thr[k]);
        gt[k] += (v.x > thr[k]) + (v.y > thr[k]) + (v.z > thr[k]) + (v.w > thr[k]);
      }
    }
  }
}

__device__ __forceinline__ int rank_lower_bound(const int* __restrict__ key, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (key[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}

// Block (x, y): the RK_TB thresholds posg[x * RK_TB ...] (grouped order, thread t holds x * RK_TB + k * RK_THREADS + t).
//   y <  Q   row chunk y of [0, N): the micro positives posg[chunk] (tp of micro), and for every class c of the block's thresholds
//            column c of keyT over the chunk (cnt per class) and the positives of class c inside the chunk (tp per class), with the
//            thresholds of the other classes masked out
//   y >= Q   share y - Q (LA elements) of the flat population keyT[0 .. N*C) (cnt of micro): nearly all of the pairs
// counts[2][N][4] += (cnt_ge, cnt_gt, tp_ge, tp_gt) at the ORIGINAL row index.
__global__ __launch_bounds__(RK_THREADS) void rank_count_kernel(const int* __restrict__ keyT, const int* __restrict__ posg,
                                                                const int* __restrict__ glab, const int* __restrict__ order, int N, int C,
                                                                int Q, int LR, int LA, int* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) int tile[RK_TILE];
  __shared__ int cls_range[2];
  const int t = threadIdx.x;
  int thr[RK_K], lab[RK_K], row[RK_K];
#pragma unroll
  for (int k = 0; k < RK_K; ++k) {
    const long long r = (long long)blockIdx.x * RK_TB + k * RK_THREADS + t;
    lab[k] = -1; row[k] = -1; thr[k] = INT_MAX;
    if (r < N) {
      const int l = glab[r];
      if (l >= 0) { lab[k] = l; row[k] = order[r]; thr[k] = posg[r]; }
    }
  }
  if ((int)blockIdx.y >= Q) {
    const long long e0 = (long long)(blockIdx.y - Q) * LA, total = (long long)N * C;
    const int len = (int)(total - e0 < LA ? total - e0 : LA);
    int ge[RK_K] = {}, gt[RK_K] = {};
    rank_stream(keyT + e0, len, thr, ge, gt, tile);
#pragma unroll
    for (int k = 0; k < RK_K; ++k)
      if (row[k] >= 0) {
        int* o = counts + (size_t)row[k] * 4;
        if (ge[k]) atomicAdd(o + 0, ge[k]);
        if (gt[k]) atomicAdd(o + 1, gt[k]);
      }
    return;
  }
  const int r0 = (int)((long long)blockIdx.y * LR < N ? (long long)blockIdx.y * LR : N), r1 = N - r0 < LR ? N : r0 + LR;
  int mge[RK_K] = {}, mgt[RK_K] = {}, cge[RK_K] = {}, cgt[RK_K] = {}, pge[RK_K] = {}, pgt[RK_K] = {};
  rank_stream(posg + r0, r1 - r0, thr, mge, mgt, tile);
  // the classes among this block's thresholds (one, or a few neighbours: the rows are grouped by label)
  if (t == 0) { cls_range[0] = INT_MAX; cls_range[1] = -1; }
  __syncthreads();
  int lo = INT_MAX, hi = -1;
#pragma unroll
  for (int k = 0; k < RK_K; ++k)
    if (lab[k] >= 0) { lo = min(lo, lab[k]); hi = max(hi, lab[k]); }
  if (hi >= 0) { atomicMin(&cls_range[0], lo); atomicMax(&cls_range[1], hi); }
  __syncthreads();
  const int c_lo = __builtin_amdgcn_readfirstlane(cls_range[0]), c_hi = __builtin_amdgcn_readfirstlane(cls_range[1]);
  for (int c = c_lo; c <= c_hi; ++c) {           // c_lo .. c_hi lie in 0 .. C-1 (valid labels only); empty when the block has no row
    int thc[RK_K];
#pragma unroll
    for (int k = 0; k < RK_K; ++k) thc[k] = lab[k] == c ? thr[k] : INT_MAX;
    rank_stream(keyT + (size_t)c * N + r0, r1 - r0, thc, cge, cgt, tile);
    const int a = max(r0, rank_lower_bound(glab, N, c)), b = min(r1, rank_lower_bound(glab, N, c + 1));
    rank_stream(posg + a, b - a, thc, pge, pgt, tile);
  }
#pragma unroll
  for (int k = 0; k < RK_K; ++k)
    if (row[k] >= 0) {
      int* o = counts + (size_t)row[k] * 4;
      if (mge[k]) atomicAdd(o + 2, mge[k]);
      if (mgt[k]) atomicAdd(o + 3, mgt[k]);
      o += (size_t)N * 4;
      if (cge[k]) atomicAdd(o + 0, cge[k]);
      if (cgt[k]) atomicAdd(o + 1, cgt[k]);
      if (pge[k]) atomicAdd(o + 2, pge[k]);
      if (pgt[k]) atomicAdd(o + 3, pgt[k]);
    }
}

}  // namespace

extern "C" long long cy_rank_ws_ints(int N, int C) {
  if (N <= 0 || C <= 0 || (long long)N * C >= (1ll << 31)) return 0;
  return (long long)N * C + 2ll * N;
}

extern "C" int cy_rank_counts(const float* scores, const long long* labels, const int* order, int N, int C, int* ws, int* counts,
                              int* correct, int* err, void* stream) {
  CY_REQUIRE(scores && labels && order && ws && counts && correct && err, "cy_rank_counts: null argument");
  CY_REQUIRE(N > 0 && C > 0, "cy_rank_counts: N=%d C=%d", N, C);
  CY_REQUIRE((long long)N * C < (1ll << 31), "cy_rank_counts: N*C = %lld does not fit the int32 counts (limit 2^31 - 1)", (long long)N * C);
  hipStream_t s = (hipStream_t)stream;
  const long long total = (long long)N * C;
  int* keyT = ws;
  int* posg = ws + total;
  int* glab = posg + N;
  rank_prep_kernel<<<(unsigned)cy_ceil_div(N, RK_THREADS), RK_THREADS, 0, s>>>(scores, labels, order, N, C, keyT, posg, glab, correct, err);
  CY_LAUNCH_CHECK("cy_rank_counts (prep)");
  // threshold blocks x (row chunks + shares of the flat population).  A share is a whole number of tiles; the target is several
  // times the blocks a CU holds at once, so that blocks are handed out as others finish (with one resident round, the CUs that
  // got one block more than the others set the time)
  hipError_t he;
  const int ncu = cyi_cu_count(&he);
  if (ncu == 0) return cy_set_error((int)he, "cy_rank_counts: cannot query the CU count: %s", hipGetErrorString(he));
  const long long nTB = cy_ceil_div(N, RK_TB);
  long long S = cy_ceil_div((long long)RK_BLOCKS_PER_CU * ncu, nTB);
  const long long tiles = cy_ceil_div(total, RK_TILE);
  if (S > tiles) S = tiles;
  long long LA = cy_ceil_div(tiles, S) * RK_TILE;
  S = cy_ceil_div(total, LA);
  if (LA > total) LA = total;                    // one share: keep it an int
  // the row chunks carry about (2 + classes per block) * N pairs per threshold against the shares' N * C
  long long Q = cy_ceil_div(6 * S, C);
  if (Q > cy_ceil_div(N, RK_TILE)) Q = cy_ceil_div(N, RK_TILE);
  const long long LR = (cy_ceil_div(N, Q) + 3) & ~3ll;
  Q = cy_ceil_div(N, LR);
  CY_REQUIRE(nTB < (1ll << 31) && Q + S <= 65535, "cy_rank_counts: grid %lld x %lld is too large", nTB, Q + S);
  rank_count_kernel<<<dim3((unsigned)nTB, (unsigned)(Q + S)), RK_THREADS, 0, s>>>(keyT, posg, glab, order, N, C, (int)Q, (int)LR, (int)LA, counts);
  CY_LAUNCH_CHECK("cy_rank_counts (count)");
  return 0;
}
