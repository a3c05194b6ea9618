// gvl_beam.hip -- beam-search decoding of the LSTM-DSA captioner on the device (wave64, gfx950).
//
// The reference's Captioner.sample reads opt['beam_size'] (pdvc/CaptioningHead/LSTM_DSA.py:132) and drops it; there is no
// reference implementation, the semantics are those of DESIGN.md section 4.3.  Two kernels:
//
//   k_beam_step    one workgroup per event row, one launch per token: per live beam ONE pass over its V logits (online
//                  max / sum exp for the log-sum-exp, a per-thread top-KW by raw logit in registers), W rounds of a workgroup
//                  arg-max (shuffles inside a wave, LDS across the waves) that leave the beam's W best logits, then the merge of
//                  the W*W survivors by score and the gather of the W recurrent state rows (h, c) by parent beam.  Correct
//                  because log_softmax subtracts a per-beam constant: the overall top W lies in the union of every beam's top W.
//   k_beam_step_lineage  the same selection (one body: beam_select) for the Transformer-DSA head, whose state is a key / value
//                  cache: instead of gathering state rows it re-orders a byte table of lineages, which the cached attention
//                  (gvl_cap_tr.hip: k_capt_attend<true>) reads its prefix through.
//   k_beam_finish  final ranking (score / len^length_penalty) and the back-trace through the recorded parents.
#include "gvl_common.hpp"

#include <float.h>
#include <math.h>

using gvl::fail;

namespace {

constexpr int kMaxBeam = 8;
constexpr int kMaxLineage = 64;               // cache positions a lineage table names
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kNoIndex = 0x7fffffff;

// (a, ia) ranks before (b, ib): the larger value, on equal values the smaller index
__device__ __forceinline__ bool before(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

template <int KW>
__device__ __forceinline__ void keep_top(float (&tv)[KW], int (&ti)[KW], float x, int idx) {
  // a thread meets its indices in ascending order, so the strict compare keeps the smaller index of equal values in front
  if (!(x > tv[KW - 1])) return;
  tv[KW - 1] = x;
  ti[KW - 1] = idx;
#pragma unroll
  for (int k = KW - 1; k > 0; --k) {
    if (tv[k] > tv[k - 1]) {
      const float fv = tv[k]; tv[k] = tv[k - 1]; tv[k - 1] = fv;
      const int fi = ti[k]; ti[k] = ti[k - 1]; ti[k - 1] = fi;
    }
  }
}

// online log-sum-exp: the running maximum moves rarely, so the sum is rescaled under a branch and every element costs one exp
__device__ __forceinline__ void lse_max(float &m, float &s, float mx) {
  if (mx > m) {
    s *= __expf(m - mx);                   // (m = -FLT_MAX at the start: s = 0 * 0)
    m = mx;
  }
}

// The selection of one token step, shared by both kernels below: leaves the step's records in global memory and the parent of every
// new beam in s_parent (W ints of the caller's LDS), behind a barrier.
// KW: capacity of the per-thread candidate list, the smallest of 1, 2, 4, 8 that holds the beam width W
template <int KW>
__device__ __forceinline__ void beam_select(const float *__restrict__ logits, int64_t ld, int V, int W,
                                            const float *__restrict__ score_in, const unsigned char *__restrict__ fin_in,
                                            float *__restrict__ score_out, unsigned char *__restrict__ fin_out,
                                            int *__restrict__ parent_out, int64_t *__restrict__ token_out,
                                            float *__restrict__ logp_out, int *__restrict__ alive, int *s_parent) {
  __shared__ float s_wm[kWaves], s_ws[kWaves];                 // per-wave max / sum exp
  __shared__ float s_rv[2][kWaves];                            // per-wave winner of an arg-max round (double-buffered)
  __shared__ int s_ri[2][kWaves];
  __shared__ float s_cv[kMaxBeam * kMaxBeam];                  // the W * W survivors: score, token log-prob, flat index
  __shared__ float s_cl[kMaxBeam * kMaxBeam];
  __shared__ int s_ci[kMaxBeam * kMaxBeam];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float kNegInf = -INFINITY;
  if (tid < W) s_parent[tid] = tid;

  for (int b = 0; b < W; ++b) {
    const float sb = score_in[(int64_t)row * W + b];
    // a finished beam offers (b, <end>) alone, score unchanged; a beam at -inf (beams 1 .. W-1 of the first step) offers nothing:
    // W finite candidates always exist beside it.  Either way uniform over the workgroup, and the beam's logits are not read
    const bool fin_b = fin_in[(int64_t)row * W + b] != 0;
    if (fin_b || sb == kNegInf) {
      if (tid < W) {
        const bool one = fin_b && tid == 0;
        s_cv[b * W + tid] = one ? sb : kNegInf;
        s_cl[b * W + tid] = 0.f;
        s_ci[b * W + tid] = one ? b * V : kNoIndex;
      }
      continue;
    }
    const float *x = logits + ((int64_t)row * W + b) * ld;
    float tv[KW];
    int ti[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k) { tv[k] = kNegInf; ti[k] = kNoIndex; }
    float m = -FLT_MAX, s = 0.f;                               // (finite: an empty thread merges as 0 * exp(0))
    // scalar head up to the first 16-byte boundary, float4 body, scalar tail: indices ascend within a thread
    int head = (int)(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) >> 2);
    if (head > V) head = V;
    const int n4 = (V - head) >> 2;
    if (tid < head) {
      const float v = x[tid];
      lse_max(m, s, v);
      s += __expf(v - m);
      keep_top<KW>(tv, ti, v, tid);
    }
    const float4 *x4 = reinterpret_cast<const float4 *>(x + head);
    for (int i = tid; i < n4; i += kThreads) {
      const float4 v = x4[i];
      const int base = head + 4 * i;
      lse_max(m, s, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
      s += (__expf(v.x - m) + __expf(v.y - m)) + (__expf(v.z - m) + __expf(v.w - m));
      keep_top<KW>(tv, ti, v.x, base);
      keep_top<KW>(tv, ti, v.y, base + 1);
      keep_top<KW>(tv, ti, v.z, base + 2);
      keep_top<KW>(tv, ti, v.w, base + 3);
    }
    {
      const int i = head + 4 * n4 + tid;
      if (i < V) {
        const float v = x[i];
        lse_max(m, s, v);
        s += __expf(v - m);
        keep_top<KW>(tv, ti, v, i);
      }
    }
    // log-sum-exp of the row
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
      const float mn = fmaxf(m, m2);
      s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
      m = mn;
    }
    if (lane == 0) { s_wm[wave] = m; s_ws[wave] = s; }
    __syncthreads();
    float mb = s_wm[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) mb = fmaxf(mb, s_wm[w]);
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) sum += s_ws[w] * __expf(s_wm[w] - mb);
    const float lse = mb + logf(sum);
    // W rounds: the workgroup's best remaining (logit, index); its owner drops it from the front of its list
    for (int j = 0; j < W; ++j) {
      float bv = tv[0];
      int bi = ti[0];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(bv, o);
        const int i2 = __shfl_xor(bi, o);
        if (before(v2, i2, bv, bi)) { bv = v2; bi = i2; }
      }
      if (lane == 0) { s_rv[j & 1][wave] = bv; s_ri[j & 1][wave] = bi; }
      __syncthreads();
      bv = s_rv[j & 1][0];
      bi = s_ri[j & 1][0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w)
        if (before(s_rv[j & 1][w], s_ri[j & 1][w], bv, bi)) { bv = s_rv[j & 1][w]; bi = s_ri[j & 1][w]; }
      if (tid == 0) {
        const bool real = bi != kNoIndex;
        const float lp = bv - lse;
        s_cv[b * W + j] = real ? sb + lp : kNegInf;
        s_cl[b * W + j] = lp;
        s_ci[b * W + j] = real ? b * V + bi : kNoIndex;
      }
      if (bi != kNoIndex && ti[0] == bi) {
#pragma unroll
        for (int k = 0; k + 1 < KW; ++k) { tv[k] = tv[k + 1]; ti[k] = ti[k + 1]; }
        tv[KW - 1] = kNegInf;
        ti[KW - 1] = kNoIndex;
      }
    }
    __syncthreads();                                           // s_wm / s_ws are rewritten by the next beam
  }
  // (a row with fewer than W candidates -- NaN logits -- leaves ended beams behind instead of unwritten records)
  if (tid < W) {
    const int64_t o = (int64_t)row * W + tid;
    score_out[o] = kNegInf; fin_out[o] = 1; parent_out[o] = tid; token_out[o] = 0; logp_out[o] = 0.f;
  }
  __syncthreads();
  // merge: the rank of a survivor is the number of survivors before it; ranks below W are the new beams, in order
  const int nc = W * W;
  if (tid < nc) {
    const float v = s_cv[tid];
    const int fi = s_ci[tid];
    int rank = 0;
    for (int k = 0; k < nc; ++k) rank += before(s_cv[k], s_ci[k], v, fi) ? 1 : 0;
    if (rank < W && fi != kNoIndex) {
      const int pb = fi / V, tok = fi - pb * V;
      const int64_t o = (int64_t)row * W + rank;
      const bool was = fin_in[(int64_t)row * W + pb] != 0;
      const bool fin = was || tok == 0;
      score_out[o] = v;
      fin_out[o] = fin ? 1 : 0;
      parent_out[o] = pb;
      token_out[o] = tok;
      logp_out[o] = s_cl[tid];
      s_parent[rank] = pb;
      if (!fin) atomicOr(alive, 1);
    }
  }
  __syncthreads();
}

template <int KW>
__global__ void __launch_bounds__(kThreads)
k_beam_step(const float *__restrict__ logits, int64_t ld, int V, int W, int H, const float *__restrict__ score_in,
            const unsigned char *__restrict__ fin_in, const float *__restrict__ h_in, const float *__restrict__ c_in,
            float *__restrict__ score_out, unsigned char *__restrict__ fin_out, int *__restrict__ parent_out,
            int64_t *__restrict__ token_out, float *__restrict__ logp_out, int *__restrict__ alive,
            float *__restrict__ h_out, float *__restrict__ c_out) {
  __shared__ int s_parent[kMaxBeam];
  beam_select<KW>(logits, ld, V, W, score_in, fin_in, score_out, fin_out, parent_out, token_out, logp_out, alive, s_parent);
  const int row = blockIdx.x, tid = threadIdx.x;
  // the recurrent state of the new beams: rows of this event re-ordered by parent, into the other pair of buffers
  const int h4 = H >> 2;
  for (int i = tid; i < W * h4; i += kThreads) {
    const int nb = i / h4, k = i - nb * h4;
    const int64_t src = ((int64_t)row * W + s_parent[nb]) * h4 + k, dst = ((int64_t)row * W + nb) * h4 + k;
    reinterpret_cast<float4 *>(h_out)[dst] = reinterpret_cast<const float4 *>(h_in)[src];
    reinterpret_cast<float4 *>(c_out)[dst] = reinterpret_cast<const float4 *>(c_in)[src];
  }
}

// The same selection for a decoder that keeps a key / value cache instead of a recurrent state: nothing of the cache moves.  Each
// beam carries a lineage, lin[r][j][q] = the slot (0 .. W-1) of event r that holds position q of beam j's prefix; the new beam j with
// parent p inherits p's lineage in front of t and names p itself at t, where p's slot has just been written.  Bytes, any alignment.
template <int KW>
__global__ void __launch_bounds__(kThreads)
k_beam_step_lineage(const float *__restrict__ logits, int64_t ld, int V, int W, const float *__restrict__ score_in,
                    const unsigned char *__restrict__ fin_in, const unsigned char *__restrict__ lin_in, int P, int t,
                    float *__restrict__ score_out, unsigned char *__restrict__ fin_out, int *__restrict__ parent_out,
                    int64_t *__restrict__ token_out, float *__restrict__ logp_out, int *__restrict__ alive,
                    unsigned char *__restrict__ lin_out) {
  __shared__ int s_parent[kMaxBeam];
  beam_select<KW>(logits, ld, V, W, score_in, fin_in, score_out, fin_out, parent_out, token_out, logp_out, alive, s_parent);
  const int row = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < W * t; i += kThreads) {                // (t = 0: nothing of lin_in is read)
    const int nb = i / t, q = i - nb * t;
    lin_out[((int64_t)row * W + nb) * P + q] = lin_in[((int64_t)row * W + s_parent[nb]) * P + q];
  }
  if (tid < W) lin_out[((int64_t)row * W + tid) * P + t] = (unsigned char)s_parent[tid];
}

// one thread per (event row, beam); a workgroup holds whole rows
__global__ void __launch_bounds__(kThreads)
k_beam_finish(const int *__restrict__ parents, const int64_t *__restrict__ tokens, const float *__restrict__ logps,
              const float *__restrict__ score, int n, int W, int T, float length_penalty, int rows_per_block,
              int64_t *__restrict__ out_tokens, float *__restrict__ out_logps, float *__restrict__ out_scores,
              int64_t *__restrict__ out_lengths) {
  __shared__ float s_rank[kThreads];
  const int tid = threadIdx.x;
  const int lr = tid / W, b = tid - lr * W;
  const int row = blockIdx.x * rows_per_block + lr;
  const bool active = lr < rows_per_block && row < n;
  const int64_t nw = (int64_t)n * W;
  int words = 0;
  float sc = 0.f;
  if (active) {
    int cur = b;
    for (int t = T - 1; t >= 0; --t) {                         // tokens after the end token are 0, before it non-zero
      const int64_t i = t * nw + (int64_t)row * W + cur;
      words += tokens[i] != 0 ? 1 : 0;
      cur = min(max(parents[i], 0), W - 1);
    }
    sc = score[(int64_t)row * W + b];
    const int len = words + 1 < T ? words + 1 : T;             // emitted tokens, the end token included
    s_rank[tid] = length_penalty == 0.f ? sc : sc / powf((float)len, length_penalty);
  }
  __syncthreads();
  if (!active) return;
  int rank = 0;
  for (int k = 0; k < W; ++k) rank += before(s_rank[lr * W + k], k, s_rank[tid], b) ? 1 : 0;
  const int64_t o = (int64_t)row * W + rank;
  out_scores[o] = sc;
  out_lengths[o] = words;
  int cur = b;
  for (int t = T - 1; t >= 0; --t) {
    const int64_t i = t * nw + (int64_t)row * W + cur;
    out_tokens[o * T + t] = tokens[i];
    out_logps[o * T + t] = logps[i];
    cur = min(max(parents[i], 0), W - 1);
  }
}

}  // namespace

extern "C" {

int gvl_beam_step_f32(const float *logits, int64_t logits_ld, int n, int W, int V, const float *score_in,
                      const unsigned char *fin_in, const float *h_in, const float *c_in, int H, float *score_out,
                      unsigned char *fin_out, int *parent_out, int64_t *token_out, float *logp_out, int *alive,
                      float *h_out, float *c_out, void *stream) {
  if (n < 0 || W < 1 || W > kMaxBeam || V < W || logits_ld < V || H <= 0 || (H & 3) || (int64_t)W * V > 0x7ffffff0)
    return fail(GVL_EINVAL, "gvl_beam_step_f32: bad sizes n=%d W=%d V=%d ld=%lld H=%d (1 <= W <= %d, W <= V, H %% 4 == 0)", n, W, V,
                (long long)logits_ld, H, kMaxBeam);
  if (n == 0) return 0;
  if (!logits || !score_in || !fin_in || !h_in || !c_in || !score_out || !fin_out || !parent_out || !token_out || !logp_out ||
      !alive || !h_out || !c_out)
    return fail(GVL_EINVAL, "gvl_beam_step_f32: null pointer");
  if (h_in == h_out || c_in == c_out || score_in == score_out || fin_in == fin_out)
    return fail(GVL_EINVAL, "gvl_beam_step_f32: the state, score and flag buffers ping-pong, nothing is updated in place");
  if ((reinterpret_cast<uintptr_t>(logits) & 3) || ((reinterpret_cast<uintptr_t>(h_in) | reinterpret_cast<uintptr_t>(c_in) |
                                                      reinterpret_cast<uintptr_t>(h_out) | reinterpret_cast<uintptr_t>(c_out)) & 15))
    return fail(GVL_EINVAL, "gvl_beam_step_f32: the state buffers must be 16-byte aligned");
  auto kern = W == 1 ? k_beam_step<1> : W == 2 ? k_beam_step<2> : W <= 4 ? k_beam_step<4> : k_beam_step<8>;
  return gvl::launch(GVL_PROF_BEAM, n, W, "k_beam_step", kern, dim3(n), dim3(kThreads), 0, (hipStream_t)stream, logits,
                     logits_ld, V, W, H, score_in, fin_in, h_in, c_in, score_out, fin_out, parent_out, token_out, logp_out, alive,
                     h_out, c_out);
}

int gvl_beam_step_lineage_f32(const float *logits, int64_t logits_ld, int n, int W, int V, const float *score_in,
                              const unsigned char *fin_in, const unsigned char *lin_in, int P, int t, float *score_out,
                              unsigned char *fin_out, int *parent_out, int64_t *token_out, float *logp_out, int *alive,
                              unsigned char *lin_out, void *stream) {
  if (n < 0 || W < 1 || W > kMaxBeam || V < W || logits_ld < V || P < 1 || P > kMaxLineage || t < 0 || t >= P ||
      (int64_t)W * V > 0x7ffffff0)
    return fail(GVL_EINVAL, "gvl_beam_step_lineage_f32: bad sizes n=%d W=%d V=%d ld=%lld P=%d t=%d (1 <= W <= %d, W <= V, "
                "0 <= t < P <= %d)", n, W, V, (long long)logits_ld, P, t, kMaxBeam, kMaxLineage);
  if (n == 0) return 0;
  if (!logits || !score_in || !fin_in || !lin_in || !score_out || !fin_out || !parent_out || !token_out || !logp_out || !alive ||
      !lin_out)
    return fail(GVL_EINVAL, "gvl_beam_step_lineage_f32: null pointer");
  if (lin_in == lin_out || score_in == score_out || fin_in == fin_out)
    return fail(GVL_EINVAL, "gvl_beam_step_lineage_f32: the lineage, score and flag buffers ping-pong, nothing is updated in place");
  if (reinterpret_cast<uintptr_t>(logits) & 3) return fail(GVL_EINVAL, "gvl_beam_step_lineage_f32: logits must be 4-byte aligned");
  auto kern = W == 1 ? k_beam_step_lineage<1> : W == 2 ? k_beam_step_lineage<2> : W <= 4 ? k_beam_step_lineage<4>
                                                                                            : k_beam_step_lineage<8>;
  return gvl::launch(GVL_PROF_BEAM_LINEAGE, n, W, "k_beam_step_lineage", kern, dim3(n), dim3(kThreads), 0, (hipStream_t)stream,
                     logits, logits_ld, V, W, score_in, fin_in, lin_in, P, t, score_out, fin_out, parent_out, token_out, logp_out,
                     alive, lin_out);
}

int gvl_beam_finish_f32(const int *parents, const int64_t *tokens, const float *logps, const float *score, int n, int W, int T,
                        float length_penalty, int64_t *out_tokens, float *out_logps, float *out_scores, int64_t *out_lengths,
                        void *stream) {
  if (n < 0 || W < 1 || W > kMaxBeam || T < 1)
    return fail(GVL_EINVAL, "gvl_beam_finish_f32: bad sizes n=%d W=%d T=%d (1 <= W <= %d)", n, W, T, kMaxBeam);
  if (n == 0) return 0;
  if (!parents || !tokens || !logps || !score || !out_tokens || !out_logps || !out_scores || !out_lengths)
    return fail(GVL_EINVAL, "gvl_beam_finish_f32: null pointer");
  const int rows_per_block = kThreads / W;
  return gvl::launch(GVL_PROF_BEAM_FINISH, n, W, "k_beam_finish", k_beam_finish, dim3((n + rows_per_block - 1) / rows_per_block),
                     dim3(kThreads), 0, (hipStream_t)stream, parents, tokens, logps, score, n, W, T, length_penalty,
                     rows_per_block, out_tokens, out_logps, out_scores, out_lengths);
}

}  // extern "C"
