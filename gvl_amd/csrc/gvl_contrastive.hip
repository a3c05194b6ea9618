// gvl_contrastive.hip -- the contrastive event-text branch (pdvc/criterion.py:269-373): cosine logits of every decoder layer, the
// InfoNCE losses and their gradient, one launch each (include/gvl_msda.h, ABI 20).
//
// Products: plain fp32 FMAs.  The cosines times set_cost_cl enter the matcher's cost and decide a DISCRETE assignment, so no operand
// is rounded below fp32; the whole branch is ~0.1 GFLOP per layer (E = 4800, G = 160, D = 128), far below what would make the
// matrix pipe worth its operand layout.  Sums over D run in chunks of 32 that are added to the total (error ~ sqrt of the length).
// No float atomics anywhere: every output element has ONE owner, cross-workgroup sums are taken by the last workgroup to arrive
// (an integer ticket) in a fixed order, so two runs are bitwise equal.
#include "gvl_common.hpp"

#include <math.h>

using gvl::fail;

namespace {

constexpr int kTile = 64;       // events x texts per workgroup of the logits kernel
constexpr int kKC = 32;         // contraction chunk
constexpr int kPad = kTile + 1; // LDS row pitch: k-major planes, odd pitch -> the transposing stores spread over the banks
constexpr float kEps = 1e-12f;  // F.normalize's clamp

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float bcast(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// (m, s) <- (m, s) (+) (m2, s2) of an online log-sum-exp; -inf maxima carry s = 0
__device__ __forceinline__ void lse_merge(float &m, float &s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) return;
  s = s * __expf(m - M) + s2 * __expf(m2 - M);
  m = M;
}
__device__ __forceinline__ void lse_push(float &m, float &s, float x) {
  if (x > m) { s = s * __expf(m - x) + 1.f; m = x; }
  else s += __expf(x - m);
}

// a logit: ONE rounded product wherever it is formed (never contracted into the subtraction that follows, so that a row of one
// element has the loss 0 exactly)
__device__ __forceinline__ float scaled(float s, float itau) {
#pragma clang fp contract(off)
  const float x = s * itau;
  return x;
}

// ---- logits ---------------------------------------------------------------------------------------------------------------------
// out[l][e][g] = <e_le, t_lg> inv_e inv_t for a 64 x 64 tile; column tiles run past G to cover the background column G.
// The squared norms of the tile's rows are accumulated beside the products, from the same LDS values in the same order by every
// thread that needs them, so that the inverse norms (written by the tile column / row 0 owners) are the ones every tile used.
template <bool VEC>
__global__ __launch_bounds__(256) void k_cl_logits(const float *__restrict__ event, const float *__restrict__ text, int64_t text_ls,
                                                   const float *__restrict__ bg, int E, int G, int D, float *__restrict__ out,
                                                   float *__restrict__ inv_e, float *__restrict__ inv_t, float *__restrict__ inv_bg) {
  __shared__ float sE[kKC][kPad];
  __shared__ float sT[kKC][kPad];
  const int l = blockIdx.z, e0 = blockIdx.x * kTile, g0 = blockIdx.y * kTile;
  const int GC = G + (bg ? 1 : 0);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const float *ev = event + (int64_t)l * E * D;
  const float *tx_ = text + (int64_t)l * text_ls;
  float acc[4][4] = {}, ne[4] = {}, nt[4] = {};
  for (int k0 = 0; k0 < D; k0 += kKC) {
    // stage: rows x 32 contraction values, transposed to k-major
    if (VEC) {
      for (int i = tid; i < kTile * (kKC / 4); i += 256) {
        const int r = i >> 3, k4 = (i & 7) * 4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (k0 + k4 < D) {                                       // (D % 4 == 0: a group of four is inside or outside)
          if (e0 + r < E) a = *reinterpret_cast<const float4 *>(ev + (int64_t)(e0 + r) * D + k0 + k4);
          const int g = g0 + r;
          if (g < G) b = *reinterpret_cast<const float4 *>(tx_ + (int64_t)g * D + k0 + k4);
          else if (g == G && bg) b = *reinterpret_cast<const float4 *>(bg + k0 + k4);
        }
        sE[k4][r] = a.x; sE[k4 + 1][r] = a.y; sE[k4 + 2][r] = a.z; sE[k4 + 3][r] = a.w;
        sT[k4][r] = b.x; sT[k4 + 1][r] = b.y; sT[k4 + 2][r] = b.z; sT[k4 + 3][r] = b.w;
      }
    } else {
      for (int i = tid; i < kTile * kKC; i += 256) {
        const int r = i >> 5, k = i & 31;
        float a = 0.f, b = 0.f;
        if (k0 + k < D) {
          if (e0 + r < E) a = ev[(int64_t)(e0 + r) * D + k0 + k];
          const int g = g0 + r;
          if (g < G) b = tx_[(int64_t)g * D + k0 + k];
          else if (g == G && bg) b = bg[k0 + k];
        }
        sE[k][r] = a;
        sT[k][r] = b;
      }
    }
    __syncthreads();
    float c[4][4] = {}, ce[4] = {}, ct[4] = {};
#pragma unroll 8
    for (int k = 0; k < kKC; ++k) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = sE[k][ty * 4 + i]; b[i] = sT[k][tx + 16 * i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ce[i] = fmaf(a[i], a[i], ce[i]);
        ct[i] = fmaf(b[i], b[i], ct[i]);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[i][j] = fmaf(a[i], b[j], c[i][j]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ne[i] += ce[i];
      nt[i] += ct[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] += c[i][j];
    }
    __syncthreads();
  }
  float ie[4], it[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ie[i] = 1.f / fmaxf(sqrtf(ne[i]), kEps);
    it[i] = 1.f / fmaxf(sqrtf(nt[i]), kEps);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = e0 + ty * 4 + i;
    if (e >= E) continue;
    if (blockIdx.y == 0 && tx == 0) inv_e[(int64_t)l * E + e] = ie[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = g0 + tx + 16 * j;
      if (g < GC) out[((int64_t)l * E + e) * GC + g] = acc[i][j] * ie[i] * it[j];
    }
  }
  if (blockIdx.x == 0 && ty == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = g0 + tx + 16 * j;
      if (g < G) inv_t[(int64_t)l * G + g] = it[j];
      else if (g == G && bg && l == 0) inv_bg[0] = it[j];
    }
  }
}

// ---- loss forward ---------------------------------------------------------------------------------------------------------------
struct ClDims {
  int L, E, G, GC, P, B, Q, NT;
  int cross, e2t, bgall;
  float itau;
};

constexpr int kRows = 64;     // events per workgroup of the loss forward

// dynamic LDS: pair_of_col[G] | vid_of_col[G] | n_v[B] (last workgroup)
__global__ __launch_bounds__(256) void k_cl_loss_fwd(const float *__restrict__ S, const int64_t *__restrict__ pair_q,
                                                     const int64_t *__restrict__ pair_t, const int64_t *__restrict__ pair_vid,
                                                     const int64_t *__restrict__ pair_tbase, ClDims d, float *__restrict__ loss,
                                                     float *__restrict__ lse_t, float *__restrict__ lse_e, int *__restrict__ ev_of_col,
                                                     int *__restrict__ col_of_ev, int *__restrict__ vid_of_col,
                                                     float *__restrict__ wcol, float *__restrict__ wev, float *__restrict__ part,
                                                     float *__restrict__ eterm, int *__restrict__ ticket) {
  extern __shared__ int smem[];
  int *s_pair = smem, *s_vid = smem + d.G, *s_nv = smem + 2 * d.G;
  __shared__ int s_evpair[kRows];
  __shared__ int s_last;
  __shared__ float s_red[256];
  const int l = blockIdx.y, tile = blockIdx.x, e0 = tile * kRows, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float *Sl = S + (int64_t)l * d.E * d.GC;
  const int64_t *pq = pair_q + (int64_t)l * d.P, *pt = pair_t + (int64_t)l * d.P;
  for (int g = tid; g < d.G; g += 256) s_pair[g] = INT_MAX;
  if (tid < kRows) s_evpair[tid] = INT_MAX;
  __syncthreads();
  for (int p = tid; p < d.P; p += 256) {
    const int64_t col = pt[p] + (pair_tbase ? pair_tbase[p] : 0), e = pair_vid[p] * d.Q + pq[p];
    if (col >= 0 && col < d.G) atomicMin(&s_pair[col], p);
    if (e >= e0 && e < e0 + kRows) atomicMin(&s_evpair[(int)(e - e0)], p);
  }
  __syncthreads();
  for (int g = tid; g < d.G; g += 256) s_vid[g] = (!d.cross && s_pair[g] != INT_MAX) ? (int)pair_vid[s_pair[g]] : -1;
  __syncthreads();
  // rows: log-sum-exp of every event over the matched texts and the background column (e2t)
  for (int r = wave; r < kRows; r += 4) {
    const int e = e0 + r;
    if (e >= d.E) break;
    const int p = s_evpair[r];
    int label = -1;
    if (p != INT_MAX) {
      const int64_t col = pt[p] + (pair_tbase ? pair_tbase[p] : 0);
      label = (col >= 0 && col < d.G) ? (int)col : -1;
    }
    float term = 0.f, lse = 0.f;
    if (d.e2t) {
      float m = -INFINITY, s = 0.f;
      for (int g = lane; g < d.GC; g += 64)
        if (g == d.G || s_pair[g] != INT_MAX) lse_push(m, s, scaled(Sl[(int64_t)e * d.GC + g], d.itau));
      const float M = wave_max(m);
      s = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - M));
      lse = M + __logf(s);
      term = lse - scaled(Sl[(int64_t)e * d.GC + (label >= 0 ? label : d.G)], d.itau);
    }
    if (lane == 0) {
      lse_e[(int64_t)l * d.E + e] = lse;
      eterm[(int64_t)l * d.E + e] = term;
      col_of_ev[(int64_t)l * d.E + e] = label;
    }
  }
  // columns: this tile's share of every text's log-sum-exp over the events (t2e)
  const int nrow = min(kRows, d.E - e0);
  for (int g = tid; g < d.G; g += 256) {
    const int vid = s_vid[g];
    float m = -INFINITY, s = 0.f;
    for (int r = 0; r < nrow; ++r) {
      const int e = e0 + r;
      if (vid < 0 || e / d.Q == vid) lse_push(m, s, scaled(Sl[(int64_t)e * d.GC + g], d.itau));
    }
    float *o = part + (((int64_t)l * d.NT + tile) * d.G + g) * 2;
    o[0] = m;
    o[1] = s;
  }
  // the last workgroup of the layer to arrive finishes the sums, in a fixed order
  __threadfence();
  __syncthreads();
  if (tid == 0) s_last = atomicAdd(&ticket[l], 1) == d.NT - 1;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  for (int v = tid; v < d.B; v += 256) s_nv[v] = 0;
  __syncthreads();
  if (!d.cross)
    for (int g = tid; g < d.G; g += 256)
      if (s_vid[g] >= 0 && s_vid[g] < d.B) atomicAdd(&s_nv[s_vid[g]], 1);
  __syncthreads();
  const float half = d.e2t ? 0.5f : 1.f;
  float t2e = 0.f;
  for (int g = tid; g < d.G; g += 256) {
    float m = -INFINITY, s = 0.f;
    for (int t = 0; t < d.NT; ++t) {
      const float *o = part + (((int64_t)l * d.NT + t) * d.G + g) * 2;
      lse_merge(m, s, __builtin_nontemporal_load(o), __builtin_nontemporal_load(o + 1));
    }
    const float lse = m + __logf(s);
    const int p = s_pair[g];
    float w = 0.f;
    int ev = -1;
    if (p != INT_MAX) ev = (int)(pair_vid[p] * d.Q + pq[p]);
    if (ev < 0 || ev >= d.E) ev = -1;              // (a pair that names no event row: ignored)
    if (ev >= 0) {
      w = d.cross ? 1.f / (float)d.P : 1.f / ((float)d.B * (float)s_nv[s_vid[g]]);
      t2e += w * (lse - scaled(Sl[(int64_t)ev * d.GC + g], d.itau));
    }
    lse_t[(int64_t)l * d.G + g] = lse;
    ev_of_col[(int64_t)l * d.G + g] = ev;
    vid_of_col[(int64_t)l * d.G + g] = s_vid[g];
    wcol[(int64_t)l * d.G + g] = w * half;
  }
  // matched events (distinct), then the e2t mean
  int cnt = 0;
  for (int e = tid; e < d.E; e += 256) cnt += __builtin_nontemporal_load(col_of_ev + (int64_t)l * d.E + e) >= 0;
  s_red[tid] = (float)cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_red[tid] += s_red[tid + o];
    __syncthreads();
  }
  const float n_match = s_red[0];
  __syncthreads();
  float e2t = 0.f;
  for (int e = tid; e < d.E; e += 256) {
    float w = 0.f;
    if (d.e2t) {
      const bool matched = __builtin_nontemporal_load(col_of_ev + (int64_t)l * d.E + e) >= 0;
      w = d.bgall ? 1.f / (float)d.E : (matched ? 1.f / n_match : 0.f);
      if (w != 0.f) e2t += w * __builtin_nontemporal_load(eterm + (int64_t)l * d.E + e);
    }
    wev[(int64_t)l * d.E + e] = w * half;
  }
  s_red[tid] = t2e;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_red[tid] += s_red[tid + o];
    __syncthreads();
  }
  t2e = s_red[0];
  __syncthreads();
  s_red[tid] = e2t;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_red[tid] += s_red[tid + o];
    __syncthreads();
  }
  e2t = s_red[0];
  if (tid == 0) {
    if (!d.cross)                                   // a video without a sentence: the mean of an empty set (criterion.py:328)
      for (int v = 0; v < d.B; ++v)
        if (s_nv[v] == 0) t2e = NAN;
    if (d.e2t && !d.bgall && n_match == 0.f) e2t = NAN;
    loss[l * 3 + 0] = d.e2t ? 0.5f * (t2e + e2t) : t2e;
    loss[l * 3 + 1] = t2e;
    loss[l * 3 + 2] = e2t;
  }
}

// ---- loss backward --------------------------------------------------------------------------------------------------------------
struct ClSaved {
  const float *S, *lse_t, *lse_e, *wcol, *wev, *gl;
  const int *ev_of_col, *col_of_ev, *vid_of_col;
};

// d loss / d cosine[l][e][g]  (g == G: the background column)
__device__ __forceinline__ float cl_ds(const ClSaved &a, const ClDims &d, int l, int e, int g) {
  const float x = scaled(a.S[((int64_t)l * d.E + e) * d.GC + g], d.itau);
  float r = 0.f;
  if (g < d.G) {
    const float wc = a.wcol[(int64_t)l * d.G + g];
    if (wc != 0.f) {
      const int vid = a.vid_of_col[(int64_t)l * d.G + g];
      if (vid < 0 || e / d.Q == vid) r += wc * __expf(x - a.lse_t[(int64_t)l * d.G + g]);
      if (e == a.ev_of_col[(int64_t)l * d.G + g]) r -= wc;
    }
  }
  const float we = a.wev[(int64_t)l * d.E + e];
  if (we != 0.f) {
    if (g == d.G || a.ev_of_col[(int64_t)l * d.G + g] >= 0) r += we * __expf(x - a.lse_e[(int64_t)l * d.E + e]);
    const int c = a.col_of_ev[(int64_t)l * d.E + e];
    if (g == (c >= 0 ? c : d.G)) r -= we;
  }
  return r * a.gl[l] * d.itau;
}

constexpr int kMaxK = 8;      // D <= 512: up to 8 values of a row per lane
constexpr int kOwn = 4;       // rows owned per wave (events) / per workgroup (texts)

// dx = inv (dxh - xh <xh, dxh>) for one row held as acc[k] over the lanes; clamped norm: the divisor was the constant 1e-12
template <int NK>
__device__ __forceinline__ void norm_backward(float (&acc)[NK], const float *__restrict__ x, float inv, int D, int lane,
                                              float *__restrict__ out) {
  float xh[NK], dot = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int dd = lane + 64 * k;
    xh[k] = dd < D ? x[dd] * inv : 0.f;
    dot = fmaf(xh[k], acc[k], dot);
  }
  dot = wave_sum(dot);
  if (inv >= 1.f / kEps) dot = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int dd = lane + 64 * k;
    if (dd < D) out[dd] = inv * (acc[k] - xh[k] * dot);
  }
}

template <int NK>
__global__ __launch_bounds__(256) void k_cl_loss_bwd(ClSaved a, ClDims d, int D, const float *__restrict__ event,
                                                     const float *__restrict__ text, int64_t text_ls, const float *__restrict__ bg,
                                                     const float *__restrict__ inv_e, const float *__restrict__ inv_t,
                                                     const float *__restrict__ inv_bg, int n_event_blocks,
                                                     float *__restrict__ grad_event, float *__restrict__ grad_text,
                                                     float *__restrict__ grad_bg) {
  __shared__ float s_sum[4][kOwn][NK * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.x < n_event_blocks) {
    // ---- role E: a wave owns 4 event rows of one layer: d ehat = sum_g ds[e][g] that_g (+ the background row)
    const int per_layer = n_event_blocks / d.L;
    const int l = blockIdx.x / per_layer, e0 = ((blockIdx.x % per_layer) * 4 + wave) * kOwn;
    if (e0 >= d.E) return;
    const float *tl = text + (int64_t)l * text_ls;
    float acc[kOwn][NK] = {};
    for (int gb = 0; gb < d.GC; gb += 64) {
      const int g = gb + lane;
      float c[kOwn];
#pragma unroll
      for (int i = 0; i < kOwn; ++i) {
        c[i] = 0.f;
        if (g < d.GC && e0 + i < d.E)
          c[i] = cl_ds(a, d, l, e0 + i, g) * (g < d.G ? inv_t[(int64_t)l * d.G + g] : inv_bg[0]);
      }
      const int n = min(64, d.GC - gb);
      for (int j = 0; j < n; ++j) {
        const float *row = (gb + j < d.G) ? tl + (int64_t)(gb + j) * D : bg;
        float v[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) v[k] = (lane + 64 * k < D) ? row[lane + 64 * k] : 0.f;
#pragma unroll
        for (int i = 0; i < kOwn; ++i) {
          const float ci = bcast(c[i], j);
#pragma unroll
          for (int k = 0; k < NK; ++k) acc[i][k] = fmaf(ci, v[k], acc[i][k]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kOwn; ++i) {
      const int e = e0 + i;
      if (e < d.E)
        norm_backward<NK>(acc[i], event + ((int64_t)l * d.E + e) * D, inv_e[(int64_t)l * d.E + e], D, lane,
                          grad_event + ((int64_t)l * d.E + e) * D);
    }
    return;
  }
  // ---- role T: a workgroup owns 4 text rows (or the background row): d that = sum_e ds[e][g] ehat_e, the waves share the
  // events; a text tensor shared by the layers (text_ls == 0) and the background row take the sum over the layers, l = 0, 1, ...
  const int tb = blockIdx.x - n_event_blocks, n_text_blocks = (d.G + kOwn - 1) / kOwn;
  const bool is_bg = tb >= n_text_blocks;
  const int g0 = is_bg ? d.G : tb * kOwn, ng = is_bg ? 1 : min(kOwn, d.G - g0);
  const bool shared = is_bg || text_ls == 0;
  float acc[kOwn][NK] = {};
  for (int l = 0; l < d.L; ++l) {
    const float *el = event + (int64_t)l * d.E * D;
    for (int eb = wave * 64; eb < d.E; eb += 256) {
      const int e = eb + lane;
      float c[kOwn];
#pragma unroll
      for (int i = 0; i < kOwn; ++i) c[i] = (e < d.E && i < ng) ? cl_ds(a, d, l, e, g0 + i) * inv_e[(int64_t)l * d.E + e] : 0.f;
      const int n = min(64, d.E - eb);
      for (int j = 0; j < n; ++j) {
        const float *row = el + (int64_t)(eb + j) * D;
        float v[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) v[k] = (lane + 64 * k < D) ? row[lane + 64 * k] : 0.f;
#pragma unroll
        for (int i = 0; i < kOwn; ++i) {
          const float ci = bcast(c[i], j);
#pragma unroll
          for (int k = 0; k < NK; ++k) acc[i][k] = fmaf(ci, v[k], acc[i][k]);
        }
      }
    }
    if (shared && l != d.L - 1) continue;
    // the four waves' shares, added in wave order; then through the normalisation
#pragma unroll
    for (int i = 0; i < kOwn; ++i)
#pragma unroll
      for (int k = 0; k < NK; ++k) s_sum[wave][i][k * 64 + lane] = acc[i][k];
    __syncthreads();
    if (wave < ng) {
      float tot[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k)
        tot[k] = ((s_sum[0][wave][k * 64 + lane] + s_sum[1][wave][k * 64 + lane]) + s_sum[2][wave][k * 64 + lane]) +
                 s_sum[3][wave][k * 64 + lane];
      const int g = g0 + wave;
      if (is_bg)
        norm_backward<NK>(tot, bg, inv_bg[0], D, lane, grad_bg);
      else
        norm_backward<NK>(tot, text + (int64_t)l * text_ls + (int64_t)g * D, inv_t[(int64_t)l * d.G + g], D, lane,
                          grad_text + (shared ? 0 : (int64_t)l * d.G * D) + (int64_t)g * D);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kOwn; ++i)
#pragma unroll
      for (int k = 0; k < NK; ++k) acc[i][k] = 0.f;
  }
}

int check_dims(const char *who, int L, int E, int G, int D) {
  if (L < 1 || E < 1 || G < 1 || D < 1 || D > 512) return fail(GVL_EINVAL, "%s: bad sizes L=%d E=%d G=%d D=%d (1 <= D <= 512, G >= 1, E >= 1)", who, L, E, G, D);
  if (G > 4096) return fail(GVL_EINVAL, "%s: G=%d beyond the kernels' range (4096)", who, G);
  if ((int64_t)L * E * (G + 1) >= (int64_t)1 << 31) return fail(GVL_EINVAL, "%s: logits tensor too large", who);
  return 0;
}

}  // namespace

extern "C" {

int gvl_cl_logits_f32(const float *event, const float *text, int64_t text_layer_stride, const float *bg, int L, int E, int G, int D,
                      float *out, float *inv_e, float *inv_t, float *inv_bg, void *stream) {
  if (int rc = check_dims("gvl_cl_logits_f32", L, E, G, D)) return rc;
  if (!event || !text || !out || !inv_e || !inv_t || (bg && !inv_bg)) return fail(GVL_EINVAL, "gvl_cl_logits_f32: null pointer");
  if (text_layer_stride != 0 && text_layer_stride < (int64_t)G * D) return fail(GVL_EINVAL, "gvl_cl_logits_f32: bad text layer stride");
  const int GC = G + (bg ? 1 : 0);
  const dim3 grid((E + kTile - 1) / kTile, (GC + kTile - 1) / kTile, L);
  const bool vec = D % 4 == 0 && text_layer_stride % 4 == 0 &&
                   ((reinterpret_cast<uintptr_t>(event) | reinterpret_cast<uintptr_t>(text) | reinterpret_cast<uintptr_t>(bg)) & 15) == 0;
  if (vec)
    return gvl::launch(GVL_PROF_CL_LOGITS, E, G, "k_cl_logits", k_cl_logits<true>, grid, dim3(256), 0, (hipStream_t)stream, event,
                       text, text_layer_stride, bg, E, G, D, out, inv_e, inv_t, inv_bg);
  return gvl::launch(GVL_PROF_CL_LOGITS, E, G, "k_cl_logits", k_cl_logits<false>, grid, dim3(256), 0, (hipStream_t)stream, event, text,
                     text_layer_stride, bg, E, G, D, out, inv_e, inv_t, inv_bg);
}

size_t gvl_cl_loss_workspace_bytes(int L, int E, int G) {
  if (L < 1 || E < 1 || G < 1) return 0;
  const size_t nt = (size_t)(E + kRows - 1) / kRows;
  // tickets (L ints, zero on entry) padded to 16 bytes | column partials | per-event terms
  return (((size_t)L * 4 + 15) / 16) * 16 + (size_t)L * nt * G * 2 * 4 + (size_t)L * E * 4;
}

int gvl_cl_loss_forward_f32(const float *logits, const int64_t *pair_q, const int64_t *pair_t, const int64_t *pair_vid,
                            const int64_t *pair_tbase, int L, int E, int G, int has_bg, int P, int B, int Q, float temperature,
                            int cross_video, int e2t, int bg_for_cl, float *loss, float *lse_t, float *lse_e, int *ev_of_col,
                            int *col_of_ev, int *vid_of_col, float *wcol, float *wev, void *workspace, size_t workspace_bytes,
                            void *stream) {
  if (int rc = check_dims("gvl_cl_loss_forward_f32", L, E, G, 1)) return rc;
  if (P < 1 || B < 1 || Q < 1 || (int64_t)B * Q != E || !(temperature > 0.f))
    return fail(GVL_EINVAL, "gvl_cl_loss_forward_f32: bad sizes P=%d B=%d Q=%d E=%d", P, B, Q, E);
  if (e2t && (!has_bg || !cross_video)) return fail(GVL_EINVAL, "gvl_cl_loss_forward_f32: e2t needs the background column and cross-video mode");
  if (!logits || !pair_q || !pair_t || !pair_vid || !loss || !lse_t || !lse_e || !ev_of_col || !col_of_ev || !vid_of_col || !wcol ||
      !wev || !workspace)
    return fail(GVL_EINVAL, "gvl_cl_loss_forward_f32: null pointer");
  if (workspace_bytes < gvl_cl_loss_workspace_bytes(L, E, G)) return fail(GVL_EINVAL, "gvl_cl_loss_forward_f32: workspace too small");
  ClDims d{L, E, G, G + (has_bg ? 1 : 0), P, B, Q, (E + kRows - 1) / kRows, cross_video != 0, e2t != 0, bg_for_cl != 0, 1.f / temperature};
  const size_t lds = ((size_t)2 * G + B) * sizeof(int);
  if (lds > 60 * 1024) return fail(GVL_EINVAL, "gvl_cl_loss_forward_f32: G=%d B=%d beyond the kernel's LDS", G, B);
  char *ws = static_cast<char *>(workspace);
  int *ticket = reinterpret_cast<int *>(ws);
  float *part = reinterpret_cast<float *>(ws + (((size_t)L * 4 + 15) / 16) * 16);
  float *eterm = part + (size_t)L * d.NT * G * 2;
  return gvl::launch(GVL_PROF_CL_LOSS_FWD, E, G, "k_cl_loss_fwd", k_cl_loss_fwd, dim3(d.NT, L), dim3(256), lds, (hipStream_t)stream,
                     logits, pair_q, pair_t, pair_vid, pair_tbase, d, loss, lse_t, lse_e, ev_of_col, col_of_ev, vid_of_col, wcol, wev,
                     part, eterm, ticket);
}

int gvl_cl_loss_backward_f32(const float *grad_loss, const float *logits, const float *lse_t, const float *lse_e, const int *ev_of_col,
                             const int *col_of_ev, const int *vid_of_col, const float *wcol, const float *wev, const float *event,
                             const float *text, int64_t text_layer_stride, const float *bg, const float *inv_e, const float *inv_t,
                             const float *inv_bg, int L, int E, int G, int D, int Q, float temperature, float *grad_event,
                             float *grad_text, float *grad_bg, void *stream) {
  if (int rc = check_dims("gvl_cl_loss_backward_f32", L, E, G, D)) return rc;
  if (Q < 1 || E % Q != 0 || !(temperature > 0.f)) return fail(GVL_EINVAL, "gvl_cl_loss_backward_f32: bad sizes Q=%d E=%d", Q, E);
  if (!grad_loss || !logits || !lse_t || !lse_e || !ev_of_col || !col_of_ev || !vid_of_col || !wcol || !wev || !event || !text ||
      !inv_e || !inv_t || !grad_event || !grad_text || (bg && (!inv_bg || !grad_bg)))
    return fail(GVL_EINVAL, "gvl_cl_loss_backward_f32: null pointer");
  ClSaved a{logits, lse_t, lse_e, wcol, wev, grad_loss, ev_of_col, col_of_ev, vid_of_col};
  ClDims d{L, E, G, G + (bg ? 1 : 0), 0, E / Q, Q, 0, 0, 0, 0, 1.f / temperature};
  const int per_layer = (E + 4 * kOwn - 1) / (4 * kOwn), n_event_blocks = per_layer * L;
  const int n_blocks = n_event_blocks + (G + kOwn - 1) / kOwn + (bg ? 1 : 0);
  const int nk = (D + 63) / 64;
#define GVL_CL_BWD(NK)                                                                                                             \
  return gvl::launch(GVL_PROF_CL_LOSS_BWD, E, G, "k_cl_loss_bwd", k_cl_loss_bwd<NK>, dim3(n_blocks), dim3(256), 0,                 \
                     (hipStream_t)stream, a, d, D, event, text, text_layer_stride, bg, inv_e, inv_t, inv_bg, n_event_blocks,       \
                     grad_event, grad_text, grad_bg)
  if (nk <= 1) GVL_CL_BWD(1);
  if (nk <= 2) GVL_CL_BWD(2);
  if (nk <= 4) GVL_CL_BWD(4);
  GVL_CL_BWD(kMaxK);
#undef GVL_CL_BWD
}

}  // extern "C"
