// bootstrap.hip — K12: the 2000-resample bootstrap ratio of medians.
//
// Replaces consensus._bootstrap_ratio (consensus.py:243-267; draw order nc then
// src, point = median(nc)/median(src)), consensus.compute_ibi_ratio
// (consensus.py:270-312; draw order src then nc, point = median(src)/median(nc))
// and the single-array chunk-shift bootstrap of pitch.estimate_pitch_chroma
// (pitch.py:143-150, seed 0).  In every case: A is drawn first, B second, and
// boot[i] = median(A*) / median(B*)  (median(A*) when B is absent).
//
// Bit-exact numpy: rng = default_rng(seed) is PCG64 (128-bit LCG, XSL-RR
// output); Generator.choice(a, n, replace=True) = integers(0, n) = Lemire's
// bounded 32-bit draw on next_uint32(), which returns the LOW then the HIGH half
// of each 64-bit output with the spare half buffered in the bit generator (so it
// carries across calls); n == 1 consumes nothing.  Resample r starts at uint32
// position s_r = sum_{q<r} consumed_q.  A Lemire rejection (probability < n / 2^32 per
// draw) is a property of the stream position and the bound alone, so the exact positions
// come from the sparse list of positions a bound-n draw would reject: the draw pass runs
// one resample per thread at r*m (counts in LDS for short jobs); a job where some resample
// consumed more than m has its stream range scanned for rejecting positions across many
// workgroups, one thread walks the resample boundaries over the sorted lists, and the
// job's resamples are drawn again from the exact starts.  The old fix-point (assume r*m,
// walk, prefix-sum, repeat until stable, inside one workgroup) remains as the fallback
// for a job whose rejection list overflows.
// Medians: the resample's multiset is kept as counts per rank of the sorted input, so
// the k-th smallest is a scan.  Percentiles use
// numpy's 'linear' method (virtual index (n-1) q, lerp with the t >= 0.5 branch),
// whose (index, gamma) the host computes with numpy's own formula.
#include "nc_block.h"
#include "nc_launch.h"
#include "nc_ws.h"

namespace nc {

typedef unsigned __int128 u128;

__device__ __forceinline__ u128 pcg_mult() {
  return ((u128)0x2360ED051FC65DA4ull << 64) | (u128)0x4385DF649FCCF645ull;
}
__device__ __forceinline__ uint64_t xsl_rr(u128 s) {
  const uint64_t x = (uint64_t)(s >> 64) ^ (uint64_t)s;
  const unsigned rot = (unsigned)(s >> 122);
  return (x >> rot) | (x << ((64u - rot) & 63u));
}
__device__ __forceinline__ u128 pcg_advance(u128 state, u128 inc, uint64_t delta) {
  u128 acc_mult = 1, acc_plus = 0, cur_mult = pcg_mult(), cur_plus = inc;
  while (delta > 0) {
    if (delta & 1) {
      acc_mult *= cur_mult;
      acc_plus = acc_plus * cur_mult + cur_plus;
    }
    cur_plus = (cur_mult + 1) * cur_plus;
    cur_mult *= cur_mult;
    delta >>= 1;
  }
  return acc_mult * state + acc_plus;
}

struct Gen32 {
  u128 s, inc;
  uint64_t out;
  int half;
  __device__ void init(u128 s0, u128 inc_, uint64_t u) {
    inc = inc_;
    s = pcg_advance(s0, inc, u / 2 + 1);
    out = xsl_rr(s);
    half = (int)(u & 1);
  }
  __device__ __forceinline__ uint32_t next() {
    uint32_t v;
    if (half) {
      v = (uint32_t)(out >> 32);
      s = s * pcg_mult() + inc;
      out = xsl_rr(s);
      half = 0;
    } else {
      v = (uint32_t)out;
      half = 1;
    }
    return v;
  }
  // Lemire bounded draw in [0, n); returns index, adds consumed uint32s
  __device__ __forceinline__ uint32_t bounded(uint32_t n, int& consumed) {
    uint64_t m = (uint64_t)next() * n;
    ++consumed;
    uint32_t left = (uint32_t)m;
    if (left < n) {
      const uint32_t thr = (uint32_t)((0xFFFFFFFFu - (n - 1)) % n);
      while (left < thr) {
        m = (uint64_t)next() * n;
        ++consumed;
        left = (uint32_t)m;
      }
    }
    return (uint32_t)(m >> 32);
  }
};

constexpr int BT = 256;    // rank / finish workgroups (small: they share CUs with the other stream)
constexpr int BD = 256;    // draw workgroups: one resample per thread
constexpr int BD_NV = 96;  // resamples with na + nb <= BD_NV keep their rank counts in LDS

__device__ __forceinline__ double lerp_np(double a, double b, double t) {
  const double d = b - a;
  return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// Per-job workspace (bootstrap_job_bytes): rank[na + nb] i32 | sorted[na + nb] f64 |
// start[n_boot] i64 | boot[n_boot] f64 | JobCtl | rejA[REJ_CAP] i64 | rejB[REJ_CAP] i64 |
// counts[n_boot][na + nb] u16 (global path)
constexpr int REJ_CAP = 512;          // rejecting positions kept per bound (expected: ~40 for n = 7000)
constexpr int64_t REJ_SLACK = 65536;  // stream positions scanned beyond n_boot * m
constexpr int SCAN_WG = 64;           // scan workgroups per job

struct JobCtl {
  int flag;    // bit 0: some resample consumed != m (set by the draw pass)
  int nrejA, nrejB;
  int status;  // 0: exact starts valid; 1: list overflow / range short; 2: redraw mismatch
  int64_t end; // stream position after the last resample
  int64_t pad;
};

struct JobWs {
  int* rankA;
  int* rankB;
  double* sortedA;
  double* sortedB;
  int64_t* start;
  double* boot;
  JobCtl* ctl;
  int* flag;
  int64_t* rejA;
  int64_t* rejB;
  uint16_t* cnt;
};

// (the host sizes this layout in bootstrap_job_bytes())
__device__ __forceinline__ JobWs job_ws(const BootArgs& a, int j, int na) {
  const int cap = a.cap[j];
  char* w = a.ws + a.ws_off[j];
  JobWs r;
  r.rankA = reinterpret_cast<int*>(w);
  r.rankB = r.rankA + na;
  r.sortedA = reinterpret_cast<double*>(w + (((size_t)cap * 4 + 15) & ~(size_t)15));
  r.sortedB = r.sortedA + na;
  r.start = reinterpret_cast<int64_t*>(r.sortedA + cap);
  r.boot = reinterpret_cast<double*>(r.start + a.n_boot);
  r.ctl = reinterpret_cast<JobCtl*>(r.boot + a.n_boot);
  r.flag = &r.ctl->flag;
  r.rejA = reinterpret_cast<int64_t*>(r.ctl + 1);
  r.rejB = r.rejA + REJ_CAP;
  r.cnt = reinterpret_cast<uint16_t*>(r.rejB + REJ_CAP);
  return r;
}

__device__ __forceinline__ bool job_skipped(const BootArgs& a, int j, int& na, int& nb) {
  na = a.a_n[j];
  nb = a.b_n ? a.b_n[j] : 0;
  return na < a.min_n || (a.b_n != nullptr && nb < a.min_n) || na <= 0;
}

// k-th smallest of a resample held as counts per rank (c[q * stride], q < n)
__device__ __forceinline__ double kth_count(const uint16_t* c, int stride, int n, int k, const double* srt) {
  int acc = 0;
  for (int q = 0; q < n; ++q) {
    acc += c[q * stride];
    if (acc > k) return srt[q];
  }
  return srt[n - 1];
}
__device__ __forceinline__ double med_count(const uint16_t* c, int stride, int n, const double* srt) {
  if (n & 1) return kth_count(c, stride, n, n / 2, srt);
  return (kth_count(c, stride, n, n / 2 - 1, srt) + kth_count(c, stride, n, n / 2, srt)) / 2.0;
}

// One resample's draws (A then B) into counts c[q * stride]; returns the uint32s consumed.
__device__ __forceinline__ int draw_resample(u128 s0, u128 inc, int64_t start, int na, int nb, bool hasB,
                                             const int* rankA, const int* rankB, uint16_t* c, int stride) {
  const int nv = na + nb;
  for (int q = 0; q < nv; ++q) c[q * stride] = 0;
  int consumed = 0;
  const bool draws = (na > 1) || (hasB && nb > 1);
  Gen32 g;
  if (draws) g.init(s0, inc, (uint64_t)start);
  if (na > 1)
    for (int q = 0; q < na; ++q) c[rankA[g.bounded((uint32_t)na, consumed)] * stride]++;
  else
    c[0] += (uint16_t)na;  // n == 1: every draw is index 0, no RNG consumed
  if (hasB) {
    if (nb > 1)
      for (int q = 0; q < nb; ++q) c[(na + rankB[g.bounded((uint32_t)nb, consumed)]) * stride]++;
    else
      c[na * stride] += (uint16_t)nb;
  }
  return consumed;
}

// Phase 1 (grid RANK_SPLIT x jobs): stable ranks and sorted values; clears the job flag.
// Element i's rank counts the values before it in sorted order, scanning the array in LDS
// tiles (every thread of a workgroup reads the same value: a broadcast), so long jobs (the
// hop-64 IBI lists of a 60-min pair, ~7 000 values) spread over RANK_SPLIT workgroups.
constexpr int RANK_SPLIT = 16;
constexpr int RANK_TILE = 2048;

__device__ __forceinline__ void rank_array(const double* X, int n, int* rank, double* sorted, double* tile) {
  const int stride = RANK_SPLIT * BT;
  for (int i0 = blockIdx.x * BT; i0 < n; i0 += stride) {
    const int i = i0 + threadIdx.x;
    const double v = i < n ? X[i] : 0.0;
    int r = 0;
    for (int t0 = 0; t0 < n; t0 += RANK_TILE) {
      const int tn = min(RANK_TILE, n - t0);
      __syncthreads();
      for (int q = threadIdx.x; q < tn; q += BT) tile[q] = X[t0 + q];
      __syncthreads();
      for (int q = 0; q < tn; ++q) {
        const double u = tile[q];
        r += (u < v) || (u == v && t0 + q < i);
      }
    }
    if (i < n) {
      rank[i] = r;
      sorted[r] = v;
    }
  }
}

__global__ __launch_bounds__(BT) void bootstrap_rank_kernel(BootArgs a) {
  __shared__ double tile[RANK_TILE];
  const int j = blockIdx.y;
  int na, nb;
  if (job_skipped(a, j, na, nb)) return;
  const JobWs w = job_ws(a, j, na);
  rank_array(a.values + a.a_off[j], na, w.rankA, w.sortedA, tile);
  if (a.b_n) rank_array(a.values + a.b_off[j], nb, w.rankB, w.sortedB, tile);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    w.ctl->flag = 0;
    w.ctl->nrejA = 0;
    w.ctl->nrejB = 0;
    w.ctl->status = 0;
  }
}

// Phase 2 (grid n_boot / BD x jobs): resample r drawn from uint32 position r * m, the
// position it has when no Lemire rejection happened before it.  A resample that
// consumes more than m flags its job.  EXACT: the pass again for flagged jobs only, from
// the starts phase 2c found; a resample whose consumption disagrees marks the job for the
// fix-point fallback.
template <bool EXACT>
__global__ __launch_bounds__(BD) void bootstrap_draw_kernel(BootArgs a) {
  __shared__ uint16_t cnt_lds[BD_NV * BD];  // [rank][thread]
  const int j = blockIdx.y;
  int na, nb;
  if (job_skipped(a, j, na, nb)) return;
  const int r = blockIdx.x * BD + threadIdx.x;
  if (r >= a.n_boot) return;
  const JobWs w = job_ws(a, j, na);
  if (EXACT && (!w.ctl->flag || w.ctl->status)) return;
  const bool hasB = a.b_n != nullptr;
  const int nv = na + nb;
  const int m = (na > 1 ? na : 0) + (nb > 1 ? nb : 0);
  const u128 s0 = ((u128)a.seed[j * 4 + 0] << 64) | (u128)a.seed[j * 4 + 1];
  const u128 inc = ((u128)a.seed[j * 4 + 2] << 64) | (u128)a.seed[j * 4 + 3];
  const bool in_lds = nv <= BD_NV;
  uint16_t* c = in_lds ? cnt_lds + threadIdx.x : w.cnt + (size_t)r * nv;
  const int stride = in_lds ? BD : 1;
  const int64_t st = EXACT ? w.start[r] : (int64_t)r * m;
  const int consumed = draw_resample(s0, inc, st, na, nb, hasB, w.rankA, w.rankB, c, stride);
  if (EXACT) {
    const int64_t nxt = r + 1 < a.n_boot ? w.start[r + 1] : w.ctl->end;
    if (st + consumed != nxt) atomicOr(&w.ctl->status, 2);
  } else if (consumed != m) {
    atomicOr(w.flag, 1);
  }
  const double ma = med_count(c, stride, na, w.sortedA);
  w.boot[r] = hasB ? ma / med_count(c + na * stride, stride, nb, w.sortedB) : ma;
}

__device__ __forceinline__ uint32_t lemire_thr(uint32_t n) { return (uint32_t)((0xFFFFFFFFu - (n - 1)) % n); }

// Phase 2b (grid SCAN_WG x jobs, flagged jobs only): every stream position p in
// [0, n_boot * m + REJ_SLACK) at which a bound-na (bound-nb) draw would be rejected:
// low32(u_p * n) < (2^32 - n) mod n.  Each thread walks a contiguous run of positions.
__global__ __launch_bounds__(BT) void bootstrap_rejscan_kernel(BootArgs a) {
  const int j = blockIdx.y;
  int na, nb;
  if (job_skipped(a, j, na, nb)) return;
  const JobWs w = job_ws(a, j, na);
  if (!w.ctl->flag) return;
  const bool hasB = a.b_n != nullptr;
  const bool ra = na > 1, rb = hasB && nb > 1;
  const int m = (ra ? na : 0) + (rb ? nb : 0);
  const int64_t total = (int64_t)a.n_boot * m + REJ_SLACK;
  const int64_t nthreads = (int64_t)SCAN_WG * BT;
  const int64_t per = ((total + nthreads - 1) / nthreads + 1) & ~(int64_t)1;
  const int64_t p0 = ((int64_t)blockIdx.x * BT + threadIdx.x) * per;
  const int64_t p1 = min(total, p0 + per);
  if (p0 >= p1) return;
  const u128 s0 = ((u128)a.seed[j * 4 + 0] << 64) | (u128)a.seed[j * 4 + 1];
  const u128 inc = ((u128)a.seed[j * 4 + 2] << 64) | (u128)a.seed[j * 4 + 3];
  const uint32_t thA = ra ? lemire_thr((uint32_t)na) : 0u, thB = rb ? lemire_thr((uint32_t)nb) : 0u;
  Gen32 g;
  g.init(s0, inc, (uint64_t)p0);
  for (int64_t p = p0; p < p1; ++p) {
    const uint32_t v = g.next();
    if (ra && (uint32_t)((uint64_t)v * (uint32_t)na) < thA) {
      const int k = atomicAdd(&w.ctl->nrejA, 1);
      if (k < REJ_CAP) w.rejA[k] = p;
    }
    if (rb && (uint32_t)((uint64_t)v * (uint32_t)nb) < thB) {
      const int k = atomicAdd(&w.ctl->nrejB, 1);
      if (k < REJ_CAP) w.rejB[k] = p;
    }
  }
}

// sorts list[0, n) (n <= REJ_CAP, distinct values) in LDS by rank
__device__ void sort_rejections(int64_t* list, int n, int64_t* tmp) {
  for (int i = threadIdx.x; i < n; i += BT) tmp[i] = list[i];
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += BT) {
    const int64_t v = tmp[i];
    int r = 0;
    for (int q = 0; q < n; ++q) r += tmp[q] < v;
    list[r] = v;
  }
  __syncthreads();
}

// Phase 2c (one workgroup per flagged job): sort the lists, then one thread walks the
// resample boundaries: a bound-n phase starting at p ends at the first e with
// e - p - (rejections in [p, e)) = n.
__global__ __launch_bounds__(BT) void bootstrap_walk_kernel(BootArgs a) {
  __shared__ int64_t tmp[REJ_CAP];
  __shared__ int64_t la[REJ_CAP], lb[REJ_CAP];
  const int j = blockIdx.x;
  int na, nb;
  if (job_skipped(a, j, na, nb)) return;
  const JobWs w = job_ws(a, j, na);
  if (!w.ctl->flag) return;
  const int ca = w.ctl->nrejA, cb = w.ctl->nrejB;
  if (ca > REJ_CAP || cb > REJ_CAP) {
    if (threadIdx.x == 0) w.ctl->status = 1;
    return;
  }
  sort_rejections(w.rejA, ca, tmp);
  sort_rejections(w.rejB, cb, tmp);
  for (int i = threadIdx.x; i < ca; i += BT) la[i] = w.rejA[i];
  for (int i = threadIdx.x; i < cb; i += BT) lb[i] = w.rejB[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  const bool hasB = a.b_n != nullptr;
  const bool ra = na > 1, rb = hasB && nb > 1;
  const int m = (ra ? na : 0) + (rb ? nb : 0);
  const int64_t total = (int64_t)a.n_boot * m + REJ_SLACK;
  int64_t p = 0;
  int ia = 0, ib = 0;
  for (int r = 0; r < a.n_boot; ++r) {
    w.start[r] = p;
    if (ra) {
      while (ia < ca && la[ia] < p) ++ia;
      int64_t e = p + na;
      while (ia < ca && la[ia] < e) {
        ++e;
        ++ia;
      }
      p = e;
    }
    if (rb) {
      while (ib < cb && lb[ib] < p) ++ib;
      int64_t e = p + nb;
      while (ib < cb && lb[ib] < e) {
        ++e;
        ++ib;
      }
      p = e;
    }
  }
  w.ctl->end = p;
  if (p > total) w.ctl->status = 1;  // the scan did not cover the whole walk
}

// Values at ranks il, il + 1, ih, ih + 1 (the +1 ranks clamped to n - 1) of v[0, n), n <= 2048,
// into q[4] in every thread; boot_out (nullable) receives v.  Keys are the order-preserving u64
// of the doubles (dkey: NaN last, as numpy sorts).  The bits every key shares are skipped, then
// one 8-bit digit per pass selects both ranks at once (two 256-bin histograms); a rank's
// neighbour is the same key while it has equal copies left, else the smallest larger key.
__device__ void boot_order_stats(const double* v, int n, int il, int ih, double* boot_out, double (&q)[4]) {
  constexpr int PER = 2048 / BT;
  __shared__ int hist[2][256];
  __shared__ unsigned long long red[2][BT / 64];
  __shared__ long long pick_d[2];
  __shared__ int pick_r[2], pick_eq[2];
  unsigned long long key[PER];
  unsigned long long kmin = ~0ull, kmax = 0ull;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int r = (int)threadIdx.x + BT * i;
    key[i] = ~0ull;
    if (r < n) {
      const double x = v[r];
      if (boot_out) boot_out[r] = x;
      key[i] = dkey(x);
      kmin = min(kmin, key[i]);
      kmax = max(kmax, key[i]);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto block_minmax = [&](unsigned long long& lo, unsigned long long& hi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, (unsigned long long)__shfl_xor((long long)lo, o, 64));
      hi = max(hi, (unsigned long long)__shfl_xor((long long)hi, o, 64));
    }
    __syncthreads();
    if (lane == 0) {
      red[0][wave] = lo;
      red[1][wave] = hi;
    }
    __syncthreads();
    lo = red[0][0];
    hi = red[1][0];
#pragma unroll
    for (int k = 1; k < BT / 64; ++k) {
      lo = min(lo, red[0][k]);
      hi = max(hi, red[1][k]);
    }
  };
  block_minmax(kmin, kmax);
  const int rank[2] = {il, ih};
  unsigned long long K[2] = {kmin, kmin};
  int rr[2] = {il, ih}, eq[2] = {n, n};
  const unsigned long long diff = kmin ^ kmax;
  if (diff) {
    const int top = 63 - __clzll((long long)diff);
    const int s0 = top & ~7;
    // keys agree on every bit above s0 + 8 (when s0 + 8 < 64)
    unsigned long long pre[2];
    pre[0] = pre[1] = s0 + 8 < 64 ? (kmin >> (s0 + 8)) << (s0 + 8) : 0ull;
    for (int shift = s0; shift >= 0; shift -= 8) {
      for (int i = threadIdx.x; i < 512; i += BT) (&hist[0][0])[i] = 0;
      __syncthreads();
      const int hs = shift + 8;
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int r = (int)threadIdx.x + BT * i;
        if (r >= n) continue;
        const unsigned long long k = key[i];
        const int d = (int)((k >> shift) & 255);
#pragma unroll
        for (int t = 0; t < 2; ++t)
          if (hs >= 64 || (k >> hs) == (pre[t] >> hs)) atomicAdd(&hist[t][d], 1);
      }
      __syncthreads();
      if (wave < 2) {  // wave t picks target t's digit: 4 bins per lane, a wave prefix scan
        const int t = wave;
        const int h0 = hist[t][4 * lane], h1 = hist[t][4 * lane + 1], h2 = hist[t][4 * lane + 2],
                  h3 = hist[t][4 * lane + 3];
        const int sum = h0 + h1 + h2 + h3;
        int incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int y = __shfl_up(incl, o, 64);
          if (lane >= o) incl += y;
        }
        const int excl = incl - sum;
        const int kk = rr[t];
        if (excl <= kk && kk < incl) {
          int r = kk - excl, d = 4 * lane, c = h0;
          if (r >= h0) {
            r -= h0;
            ++d;
            c = h1;
            if (r >= h1) {
              r -= h1;
              ++d;
              c = h2;
              if (r >= h2) {
                r -= h2;
                ++d;
                c = h3;
              }
            }
          }
          pick_d[t] = d;
          pick_r[t] = r;
          pick_eq[t] = c;
        }
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        pre[t] |= (unsigned long long)pick_d[t] << shift;
        rr[t] = pick_r[t];
        eq[t] = pick_eq[t];
      }
      __syncthreads();
    }
    K[0] = pre[0];
    K[1] = pre[1];
  } else {
    rr[0] = il;
    rr[1] = ih;
  }
  // neighbours: the smallest key above each selected one (both at once)
  unsigned long long nx0 = ~0ull, nx1 = ~0ull;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int r = (int)threadIdx.x + BT * i;
    if (r >= n) continue;
    if (key[i] > K[0]) nx0 = min(nx0, key[i]);
    if (key[i] > K[1]) nx1 = min(nx1, key[i]);
  }
  unsigned long long neg1 = ~nx1;  // block_minmax takes a min and a max: max of ~x = ~min of x
  block_minmax(nx0, neg1);
  const unsigned long long nx[2] = {nx0, ~neg1};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const bool same = rank[t] + 1 >= n || rr[t] + 1 < eq[t];
    q[2 * t] = dunkey(K[t]);
    q[2 * t + 1] = same ? q[2 * t] : dunkey(nx[t]);
  }
}

// Phase 3 (one workgroup per job): for a flagged job the exact resample positions by a
// fix-point (assume r * m, walk, prefix-sum the consumed counts, repeat until stable) and
// the boot values again; then the bitonic sort of the boot values, percentiles, point.
__global__ __launch_bounds__(BT) void bootstrap_finish_kernel(BootArgs a) {
  __shared__ BlockScratch<BT> bs;
  __shared__ int sh_changed;
  const int j = blockIdx.x;
  int na, nb;
  if (job_skipped(a, j, na, nb)) {
    if (threadIdx.x == 0) {
      a.point_out[j] = NAN;
      a.lo_out[j] = NAN;
      a.hi_out[j] = NAN;
    }
    return;
  }
  const JobWs w = job_ws(a, j, na);
  const bool hasB = a.b_n != nullptr;
  const int nv = na + nb;
  if (w.ctl->flag && w.ctl->status) {  // fallback: the exact-start pass could not be used
    const u128 s0 = ((u128)a.seed[j * 4 + 0] << 64) | (u128)a.seed[j * 4 + 1];
    const u128 inc = ((u128)a.seed[j * 4 + 2] << 64) | (u128)a.seed[j * 4 + 3];
    const int m = (na > 1 ? na : 0) + (nb > 1 ? nb : 0);
    for (int r = threadIdx.x; r < a.n_boot; r += BT) w.start[r] = (int64_t)r * m;
    __syncthreads();
    for (int iter = 0; iter < 4096; ++iter) {
      int local_cons[(2048 + BT - 1) / BT];
      int li = 0;
      for (int r = threadIdx.x; r < a.n_boot; r += BT, ++li)
        local_cons[li] = draw_resample(s0, inc, w.start[r], na, nb, hasB, w.rankA, w.rankB,
                                       w.cnt + (size_t)r * nv, 1);
      if (threadIdx.x == 0) sh_changed = 0;
      __syncthreads();
      int64_t carry = 0;
      for (int base = 0, l2 = 0; base < a.n_boot; base += BT, ++l2) {
        const int r = base + threadIdx.x;
        const int v = r < a.n_boot ? local_cons[l2] : 0;
        int tot = 0;
        const int ex = block_exclusive_scan<BT>(v, tot, bs);
        if (r < a.n_boot) {
          const int64_t ns = carry + ex;
          if (ns != w.start[r]) {
            w.start[r] = ns;
            sh_changed = 1;
          }
        }
        carry += tot;
        __syncthreads();
      }
      __syncthreads();
      if (!sh_changed) break;
      __syncthreads();
    }
    for (int r = threadIdx.x; r < a.n_boot; r += BT) {
      const uint16_t* c = w.cnt + (size_t)r * nv;
      const double ma = med_count(c, 1, na, w.sortedA);
      w.boot[r] = hasB ? ma / med_count(c + na, 1, nb, w.sortedB) : ma;
    }
    __syncthreads();
  }
  // the four order statistics numpy's percentile reads (ranks il, il + 1, ih, ih + 1 of the
  // sorted boot values) by a two-target radix select over the values held in registers (round 5:
  // the 2048-element bitonic sort it replaces was 66 barrier phases, 0.50 ms per bench step)
  const int il = (int)a.idx_lo, ih = (int)a.idx_hi;
  double q[4];
  boot_order_stats(w.boot, a.n_boot, il, ih, a.boot_out ? a.boot_out + (size_t)j * a.n_boot : nullptr, q);
  if (threadIdx.x == 0) {
    a.lo_out[j] = lerp_np(q[0], q[1], a.g_lo);
    a.hi_out[j] = lerp_np(q[2], q[3], a.g_hi);
    const double pa = (na & 1) ? w.sortedA[na / 2] : (w.sortedA[na / 2 - 1] + w.sortedA[na / 2]) / 2.0;
    double pb = 1.0;
    if (hasB) pb = (nb & 1) ? w.sortedB[nb / 2] : (w.sortedB[nb / 2 - 1] + w.sortedB[nb / 2]) / 2.0;
    a.point_out[j] = hasB ? pa / pb : pa;
  }
}

// one job's region, as job_ws() reads it on the device, closed to 256 bytes
size_t bootstrap_job_bytes(int cap, int n_boot) {
  WsCarve c;
  c.skip((size_t)cap * sizeof(int), 16);                        // rank
  c.skip((size_t)cap * sizeof(double), 8);                      // sorted
  c.skip((size_t)n_boot * sizeof(int64_t), 8);                  // start
  c.skip((size_t)n_boot * sizeof(double), 8);                   // boot
  c.skip(sizeof(JobCtl) + 2 * REJ_CAP * sizeof(int64_t), 8);    // JobCtl, rejA, rejB
  c.skip((size_t)n_boot * cap * sizeof(uint16_t), 2);           // counts
  c.skip(0);
  return c.bytes();
}

int launch_bootstrap(const BootArgs& a, int n_jobs, hipStream_t st) {
  if (n_jobs <= 0) return 0;
  if (a.n_boot > 2048 || a.n_boot < 1) {
    set_error("bootstrap: n_boot must be in [1, 2048]");
    return -2;
  }
  hipLaunchKernelGGL(bootstrap_rank_kernel, dim3(RANK_SPLIT, n_jobs), dim3(BT), 0, st, a);
  const dim3 gd((a.n_boot + BD - 1) / BD, n_jobs);
  hipLaunchKernelGGL(bootstrap_draw_kernel<false>, gd, dim3(BD), 0, st, a);
  hipLaunchKernelGGL(bootstrap_rejscan_kernel, dim3(SCAN_WG, n_jobs), dim3(BT), 0, st, a);
  hipLaunchKernelGGL(bootstrap_walk_kernel, dim3(n_jobs), dim3(BT), 0, st, a);
  hipLaunchKernelGGL(bootstrap_draw_kernel<true>, gd, dim3(BD), 0, st, a);
  hipLaunchKernelGGL(bootstrap_finish_kernel, dim3(n_jobs), dim3(BT), 0, st, a);
  NC_HIP(hipGetLastError());
  return 0;
}

}  // namespace nc
