// Sign tracks for the streaming detector (gfx950): the step behind pack_detections_kernel that turns the per-frame box list of
// serve.SignDetector into tracks with an id, a class voted over the frames seen so far and a hit count.  The rule is in
// include/capsyolo_hip.h (cy_track_update) and restated in numpy in tests/track_ref.py.
//   track_update_kernel   ONE block of 256 threads per frame: candidate table (predicted box x detection) in LDS, greedy assignment
//                         with one block arg-max per round, track update, births, class evidence, record
// The kernel is a chain of small dependent steps (latency, not throughput): one launch, one barrier per greedy round, no atomics to
// global memory.  Thread t owns track slot t from the first load to the last store; a wave owns a track's class evidence.
#include "common.h"
#include "box_iou.h"

#include <limits.h>

// the double arithmetic on boxes and the float arithmetic on class evidence restate numpy expressions operation by operation: no
// fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int TRK_THREADS = 256, TRK_WAVES = TRK_THREADS / 64;
constexpr int TRK_MAX_TRACKS = TRK_THREADS;       // thread t owns slot t
constexpr int TRK_MAX_PAIRS = 4096;               // the candidate table: 32 KiB of the 48 KiB a launch gets without opting in

// the state buffer: header, T slots, then the class evidence float [T][C].  All zero = no track, frame 0, no id handed out.
struct trk_header_t { int frame, next_id, pad[6]; };
struct trk_slot_t {
  double xy[4], vel[4];
  int id, age, hits, misses;
  float conf;
  int pad[3];
};
static_assert(sizeof(trk_header_t) == 32 && sizeof(trk_slot_t) == 96, "the state layout");
// a slot in registers (no padding words to carry along)
struct trk_regs_t {
  double xy[4], vel[4];
  int id, age, hits, misses;
  float conf;
};
static_assert(sizeof(cy_tracks_header_t) == 32 && sizeof(cy_track_t) == 64, "the record layout of include/capsyolo_hip.h");

// what happens to a slot's class evidence in this call (LDS word of the slot: detection << 3 | kind)
enum { EV_FREE = 0, EV_KEEP = 1, EV_MATCH = 2, EV_BORN = 3, EV_DIED = 4 };

// LDS besides the candidate table: per track the predicted box, the matched detection, the detection born into the r-th free slot
// and the evidence word; per detection a state byte
constexpr size_t TRK_LDS_PER_TRACK = 4 * sizeof(double) + 3 * sizeof(int);
__host__ __device__ constexpr size_t trk_lds_bytes(int K, int T) {
  return ((size_t)K * T * sizeof(double) + (size_t)T * TRK_LDS_PER_TRACK + (size_t)K + 7) & ~(size_t)7;
}
static_assert(trk_lds_bytes(TRK_MAX_PAIRS / TRK_MAX_TRACKS, TRK_MAX_TRACKS) + 256 <= 48 * 1024, "T = 256 at the pair cap");
static_assert(trk_lds_bytes(TRK_MAX_PAIRS, 1) + 256 <= 48 * 1024, "T = 1 at the pair cap");

enum { DET_DEAD = 0, DET_LIVE = 1, DET_MATCHED = 2 };

// Exclusive rank of this thread among the block's threads with `flag`, and their number.  One barrier; `scratch` has TRK_WAVES
// words, and two calls in a row must use different scratch (a slow thread may still be reading the first).
__device__ __forceinline__ int trk_block_rank(bool flag, int* scratch, int* total) {
  const unsigned long long mask = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) scratch[wave] = __popcll(mask);
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < TRK_WAVES; ++w) { const int c = scratch[w]; all += c; if (w < wave) before += c; }
  *total = all;
  return before + __popcll(mask & ((1ull << lane) - 1ull));
}

// is class score (av, ai) ahead of (bv, bi) in np.argmax's order?  The first maximum wins and a NaN counts as the maximum (so the
// first NaN wins); index INT_MAX: no score at all
__device__ __forceinline__ bool trk_score_ahead(float av, int ai, float bv, int bi) {
  if (ai == INT_MAX) return false;
  if (bi == INT_MAX) return true;
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return an && (!bn || ai < bi);
  return av > bv || (av == bv && ai < bi);
}

__global__ __launch_bounds__(TRK_THREADS) void track_update_kernel(const int* __restrict__ count, const double* __restrict__ box_xy,
                                                                   const float* __restrict__ conf, const int* __restrict__ rect,
                                                                   const float* __restrict__ scores, int K, int C, int T, double iou_th,
                                                                   int max_misses, int min_hits, float decay, int motion,
                                                                   trk_header_t* __restrict__ sh, trk_slot_t* __restrict__ st,
                                                                   float* __restrict__ evid, cy_tracks_header_t* __restrict__ rh,
                                                                   cy_track_t* __restrict__ rec, int* __restrict__ det_track) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* table = sm;                                       // [T][K]: the IoU of a candidate pair, -1 for every other pair
  double* pred = table + (size_t)K * T;                     // [T][4]
  int* match = (int*)(pred + (size_t)T * 4);                // [T]: -2 free slot, -1 live and unmatched, else its detection
  int* born_det = match + T;                                // [T]: the r-th unmatched detection (r below the free slots)
  int* evk = born_det + T;                                  // [T]
  unsigned char* dstate = (unsigned char*)(evk + T);        // [K]
  __shared__ double red_v[2][TRK_WAVES];
  __shared__ int red_e[2][TRK_WAVES];
  __shared__ int rank_scratch[2][TRK_WAVES];
  __shared__ int counters[3];                               // live, confirmed, deaths

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cnt = *count;
  const int n = cnt < 0 ? 0 : (cnt < K ? cnt : K);
  const int frame0 = sh->frame, next_id0 = sh->next_id;
  const int KT = K * T;

  // ---- this thread's slot, its predicted box; the detections that take part
  trk_regs_t my = {};
  bool live0 = false;
  if (tid < T) {
    const trk_slot_t* in = st + tid;
    for (int k = 0; k < 4; ++k) { my.xy[k] = in->xy[k]; my.vel[k] = in->vel[k]; }
    my.id = in->id; my.age = in->age; my.hits = in->hits; my.misses = in->misses; my.conf = in->conf;
    live0 = my.id != 0;
    if (live0)
      for (int k = 0; k < 4; ++k) pred[4 * tid + k] = motion ? my.xy[k] + my.vel[k] : my.xy[k];
    match[tid] = live0 ? -1 : -2;
  }
  for (int s = tid; s < K; s += TRK_THREADS)
    dstate[s] = (s < n && (rect[4 * s] | rect[4 * s + 1] | rect[4 * s + 2] | rect[4 * s + 3])) ? DET_LIVE : DET_DEAD;
  if (tid < 3) counters[tid] = 0;
  __syncthreads();

  // ---- the candidate table.  Entry e = t K + s belongs to thread e mod 256 from here to the end of the assignment: nobody else
  // reads or writes it, so the table itself needs no barrier
  for (int e = tid; e < KT; e += TRK_THREADS) {
    const int t = e / K, s = e - t * K;
    double v = -1.0;
    if (match[t] == -1 && dstate[s] == DET_LIVE) {
      const double iou = box_iou(pred + 4 * t, box_xy + 4 * (size_t)s);
      if (iou > iou_th) v = iou;                            // strictly; false for a NaN.  A candidate is > iou_th >= 0
    }
    table[e] = v;
  }

  // ---- greedy assignment: the largest IoU among the pairs whose track and detection are free, ties to the lower e (the lower
  // track slot, then the lower detection slot).  A round's winner is struck from the table by the next round's scan.
  int lt = -1, ls = -1;
  for (int round = 0;; ++round) {
    double bv = -1.0;
    int be = INT_MAX;
    for (int e = tid; e < KT; e += TRK_THREADS) {
      const double v = table[e];
      if (v < 0.0) continue;
      if (lt >= 0) {
        const int t = e / K, s = e - t * K;
        if (t == lt || s == ls) { table[e] = -1.0; continue; }
      }
      if (v > bv) { bv = v; be = e; }                       // (e ascends: the first of equal values stays)
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const double ov = __shfl_xor(bv, off);
      const int oe = __shfl_xor(be, off);
      if (ov > bv || (ov == bv && oe < be)) { bv = ov; be = oe; }
    }
    if (lane == 0) { red_v[round & 1][wave] = bv; red_e[round & 1][wave] = be; }
    __syncthreads();            // (the other half of red_* is written next: everybody has read it before this barrier)
    bv = red_v[round & 1][0]; be = red_e[round & 1][0];
    for (int w = 1; w < TRK_WAVES; ++w) {
      const double ov = red_v[round & 1][w];
      const int oe = red_e[round & 1][w];
      if (ov > bv || (ov == bv && oe < be)) { bv = ov; be = oe; }
    }
    if (bv < 0.0) break;        // no candidate left (the same answer in every thread)
    lt = be / K; ls = be - lt * K;
    if (tid == 0) { match[lt] = ls; dstate[ls] = DET_MATCHED; }
  }
  __syncthreads();

  // ---- matched and unmatched live tracks
  int kind = EV_FREE, src = 0, detf = 0;
  bool died = false;
  if (live0) {
    const int m = match[tid];
    if (m >= 0) {
      for (int k = 0; k < 4; ++k) {
        const double d = box_xy[4 * (size_t)m + k];
        my.vel[k] = d - my.xy[k];
        my.xy[k] = d;
      }
      my.conf = conf[m];
      my.hits += 1;
      my.misses = 0;
      detf = m; kind = EV_MATCH; src = m;
      det_track[m] = my.id;
    } else {
      my.misses += 1;
      detf = -1; kind = EV_KEEP;
      if (motion)
        for (int k = 0; k < 4; ++k) my.xy[k] = my.xy[k] + my.vel[k];
      if (my.misses > max_misses) { my = trk_regs_t{}; detf = 0; kind = EV_DIED; died = true; }
    }
  }

  // ---- births: the r-th unmatched live detection, in slot order, goes into the r-th free slot, in slot order
  const bool free_now = tid < T && my.id == 0;
  int n_free;
  const int free_rank = trk_block_rank(free_now, rank_scratch[0], &n_free);
  int unmatched = 0;
  for (int s0 = 0, pass = 1; s0 < K; s0 += TRK_THREADS, ++pass) {
    const int s = s0 + tid;
    const bool unm = s < K && dstate[s] == DET_LIVE;
    int here;
    const int r = unmatched + trk_block_rank(unm, rank_scratch[pass & 1], &here);
    if (s < K && dstate[s] != DET_MATCHED) det_track[s] = unm && r < n_free ? next_id0 + r + 1 : 0;
    if (unm && r < n_free) born_det[r] = s;
    unmatched += here;
  }
  const int births = unmatched < n_free ? unmatched : n_free;
  __syncthreads();
  if (free_now && free_rank < births) {
    const int s = born_det[free_rank];
    for (int k = 0; k < 4; ++k) { my.xy[k] = box_xy[4 * (size_t)s + k]; my.vel[k] = 0.0; }
    my.id = next_id0 + free_rank + 1;
    my.conf = conf[s];
    my.hits = 1; my.misses = 0; my.age = 0;
    detf = s; kind = EV_BORN; src = s;
  }

  // ---- age, the slot's state and its record (class and score follow below), the counts of the header
  if (tid < T) {
    const bool live = my.id != 0;
    if (live) my.age += 1;
    evk[tid] = (src << 3) | kind;
    trk_slot_t* o = st + tid;
    for (int k = 0; k < 4; ++k) { o->xy[k] = my.xy[k]; o->vel[k] = my.vel[k]; }
    o->id = my.id; o->age = my.age; o->hits = my.hits; o->misses = my.misses; o->conf = my.conf;
    o->pad[0] = o->pad[1] = o->pad[2] = 0;
    cy_track_t r;
    for (int k = 0; k < 4; ++k) r.xy[k] = my.xy[k];
    r.id = my.id; r.cls = 0; r.age = my.age; r.hits = my.hits; r.misses = my.misses; r.det = detf;
    r.conf = my.conf; r.score = 0.f;
    rec[tid] = r;
    if (live) atomicAdd(&counters[0], 1);                   // (LDS)
    if (live && my.hits >= min_hits) atomicAdd(&counters[1], 1);
    if (died) atomicAdd(&counters[2], 1);
  }
  __syncthreads();
  if (tid == 0) {
    sh->frame = frame0 + 1;
    sh->next_id = next_id0 + births;
    rh->frame = frame0 + 1; rh->live = counters[0]; rh->confirmed = counters[1]; rh->births = births; rh->deaths = counters[2];
    rh->dropped = unmatched - births; rh->next_id = next_id0 + births; rh->err = 0;
  }

  // ---- class evidence, one wave per track: the update, then np.argmax over the C sums
  for (int t = wave; t < T; t += TRK_WAVES) {
    const int code = evk[t], k = code & 7;
    if (k == EV_FREE) continue;
    float* ev = evid + (size_t)t * C;
    if (k == EV_DIED) {
      for (int c = lane; c < C; c += 64) ev[c] = 0.f;
      continue;
    }
    const float* sc = scores + (size_t)(code >> 3) * C;
    float bv = 0.f;
    int bi = INT_MAX;
    for (int c = lane; c < C; c += 64) {
      float x;
      if (k == EV_MATCH) {
        const float kept = decay * ev[c];
        x = kept + sc[c];
      } else if (k == EV_BORN) {
        x = sc[c];
      } else {
        x = ev[c];
      }
      if (k != EV_KEEP) ev[c] = x;
      if (trk_score_ahead(x, c, bv, bi)) { bv = x; bi = c; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (trk_score_ahead(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { rec[t].cls = bi; rec[t].score = bv; }
  }
}

}  // namespace

#define CY_S ((hipStream_t)stream)

extern "C" int cy_track_max_pairs(void) { return TRK_MAX_PAIRS; }

extern "C" long long cy_track_state_bytes(int max_tracks, int n_classes) {
  if (max_tracks < 1 || n_classes < 1) return 0;
  return (long long)sizeof(trk_header_t) + (long long)max_tracks * (long long)sizeof(trk_slot_t) +
         (long long)max_tracks * n_classes * (long long)sizeof(float);
}

extern "C" int cy_track_update(const int* count, const double* box_xy, const float* conf, const int* rect, const float* scores, int K,
                               int C, int max_tracks, double iou_th, int max_misses, int min_hits, float decay, int motion, void* state,
                               void* record, void* stream) {
  CY_REQUIRE(count && box_xy && conf && rect && scores && state && record,
             "cy_track_update: null argument (count, box_xy, conf, rect, scores, state, record)");
  CY_REQUIRE(max_tracks >= 1 && max_tracks <= TRK_MAX_TRACKS, "cy_track_update: max_tracks=%d is not in 1..%d", max_tracks, TRK_MAX_TRACKS);
  CY_REQUIRE(K >= 1, "cy_track_update: K=%d slots", K);
  CY_REQUIRE((long long)K * max_tracks <= TRK_MAX_PAIRS,
             "cy_track_update: K=%d slots x max_tracks=%d is %lld pairs, the candidate table holds %d (cy_track_max_pairs)", K, max_tracks,
             (long long)K * max_tracks, TRK_MAX_PAIRS);
  CY_REQUIRE(C >= 1, "cy_track_update: C=%d class scores per slot", C);
  CY_REQUIRE(iou_th >= 0.0 && iou_th <= 1.0, "cy_track_update: iou_th=%g is not in [0, 1]", iou_th);     // also NaN
  CY_REQUIRE(max_misses >= 0, "cy_track_update: max_misses=%d", max_misses);
  CY_REQUIRE(min_hits >= 1, "cy_track_update: min_hits=%d", min_hits);
  CY_REQUIRE(decay >= 0.f && decay <= 1.f, "cy_track_update: decay=%g is not in [0, 1]", (double)decay);
  CY_REQUIRE(motion == 0 || motion == 1, "cy_track_update: motion=%d is not 0 or 1", motion);
  CY_REQUIRE(((uintptr_t)state & 7) == 0 && ((uintptr_t)record & 7) == 0,
             "cy_track_update: the state and record buffers must be 8-byte aligned");
  const int T = max_tracks;
  trk_header_t* sh = (trk_header_t*)state;
  trk_slot_t* st = (trk_slot_t*)(sh + 1);
  float* evid = (float*)(st + T);
  cy_tracks_header_t* rh = (cy_tracks_header_t*)record;
  cy_track_t* rec = (cy_track_t*)(rh + 1);
  int* det_track = (int*)(rec + T);
  track_update_kernel<<<1, TRK_THREADS, trk_lds_bytes(K, T), CY_S>>>(count, box_xy, conf, rect, scores, K, C, T, iou_th, max_misses, min_hits,
                                                                     decay, motion, sh, st, evid, rh, rec, det_track);
  CY_LAUNCH_CHECK("cy_track_update");
  return 0;
}
