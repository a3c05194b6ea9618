// gvl_cap_tr.hip -- the token step of the Transformer-DSA caption head's greedy decoding over a KV cache (wave64, gfx950).
//
// The reference decodes without a cache: for every token it runs the whole prefix through every layer again
// (pdvc/CaptioningHead/Transformer_DSA.py:226-238).  The head is strictly causal, so position t of a layer depends on positions
// 0..t of the layer below only: here a token is ONE new position per row, its keys and values appended to a per-layer cache.
//
//   k_capt_embed   x[r] = embed[it[r]] + pos_table[t]  (:201-206; rows beyond the table stay zero) and max |x[r]|, the row scale
//                  the split-fp16 Linear behind it reads.  One wavefront per row.
//   k_capt_attend  BertSelfAttention for the new position (:95-99) + residual + norm1: one workgroup per row, one wavefront per
//                  head (D = 64).  A wavefront's 16-byte loads cover FOUR cached positions of its head at a time (16 lanes x
//                  float4 = 64 channels): K and V go from memory straight to registers, each quarter-wave keeps an online softmax
//                  over its positions (t, t - 4, ...), the four are merged by shuffles.  Position t itself is taken from the
//                  projection's output row, never read back from the cache; no position behind t is touched.  LayerNorm
//                  statistics over the H heads go through LDS (two passes: mean, then the centred sum of squares).
//                  Plain fp32 FMAs: the step is a read of (t + 1) x 2 x 256 bytes per head, the matrix cores have nothing to do.
//                  k_capt_attend<true> is the same step for beam search: position p < t comes from the slot the row's lineage names.
#include "gvl_common.hpp"

#include <math.h>

using gvl::fail;

namespace {

constexpr int kHeadDim = 64;
constexpr int kMaxHeads = 8;
constexpr int kMaxPositions = 64;
constexpr int kMaxBeam = 8;

__global__ void __launch_bounds__(64)
k_capt_embed(const float *__restrict__ embed, int n_vocab, const float *__restrict__ pos_table, int pos_rows,
             const int64_t *__restrict__ it, int t, int C, float *__restrict__ x, float *__restrict__ amax) {
  const int row = blockIdx.x, lane = threadIdx.x;
  int64_t tok = it[row];
  tok = tok < 0 ? 0 : (tok >= n_vocab ? n_vocab - 1 : tok);          // (an id outside the table never becomes an address)
  const bool has_pos = t < pos_rows;
  float m = 0.f;
  for (int c4 = lane; c4 < C / 4; c4 += 64) {
    float4 v = ld4(embed, tok * (C / 4) + c4);
    if (has_pos) {
      const float4 p = ld4(pos_table, (int64_t)t * (C / 4) + c4);
      v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
    }
    st4(x, (int64_t)row * (C / 4) + c4, v);
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) amax[row] = m;
}

// merge two online-softmax states (m, s, acc) <- (m, s, acc) + (m2, s2, acc2); a state that has seen nothing carries m = -inf, s = 0
__device__ __forceinline__ void merge(float &m, float &s, float4 &a, float m2, float s2, float4 a2) {
  const float mn = fmaxf(m, m2);
  const float f1 = m == -INFINITY ? 0.f : expf(m - mn), f2 = m2 == -INFINITY ? 0.f : expf(m2 - mn);
  s = s * f1 + s2 * f2;
  a.x = a.x * f1 + a2.x * f2; a.y = a.y * f1 + a2.y * f2; a.z = a.z * f1 + a2.z * f2; a.w = a.w * f1 + a2.w * f2;
  m = mn;
}

// kBeam: the rows are n / W events of W beams (beam search, gvl_beam.hip: k_beam_step_lineage).  A row still appends position t at
// its OWN slot, but reads position p < t from the slot of its event that lineage[row][p] names -- the cache is never copied by
// parent.  A quarter-wave's sixteen loads are one position of one head, so the slot is one base address per quarter-wave and
// position; the row's lineage (Tc <= 64 bytes) is fetched once, one byte per lane, and handed out by a shuffle per position.
template <bool kBeam>
__global__ void __launch_bounds__(64 * kMaxHeads)
k_capt_attend(const float *__restrict__ qkv, int64_t ld_qkv, const float *__restrict__ xres, int64_t ld_x,
              float *__restrict__ cache, const unsigned char *__restrict__ lineage, int W, int n, int Tc, int t, int H,
              const float *__restrict__ gamma, const float *__restrict__ beta, float eps, float *__restrict__ out,
              float *__restrict__ amax_out) {
  __shared__ float s_part[kMaxHeads];
  __shared__ float s_part2[kMaxHeads];
  __shared__ float s_max[kMaxHeads];
  const int row = blockIdx.x, lane = threadIdx.x & 63, head = threadIdx.x >> 6;        // blockDim.x = 64 H
  const int sub = lane >> 4, chunk = lane & 15;                                         // position of the four, float4 of the 16
  const int C = H * kHeadDim;
  const int col = head * kHeadDim + 4 * chunk;
  const float *qrow = qkv + (int64_t)row * ld_qkv;
  const float4 q = *reinterpret_cast<const float4 *>(qrow + col);
  const float4 k_new = *reinterpret_cast<const float4 *>(qrow + C + col);
  const float4 v_new = *reinterpret_cast<const float4 *>(qrow + 2 * C + col);
  float *kc = cache + ((int64_t)row * Tc) * C + col;                                   // K of this row, position 0
  float *vc = kc + (int64_t)n * Tc * C;                                                // V
  if (sub == 0) {                                                                      // append position t
    *reinterpret_cast<float4 *>(kc + (int64_t)t * C) = k_new;
    *reinterpret_cast<float4 *>(vc + (int64_t)t * C) = v_new;
  }
  int slot = 0;                                                                        // lane p: the slot of position p, p < t
  int64_t to_event = 0;                                                                // from this row's slot to slot 0 of its event
  if (kBeam) {
    if (lane < t) slot = min((int)lineage[(int64_t)row * Tc + lane], W - 1);           // (clamped: never an address outside the event)
    to_event = -(int64_t)(row % W) * Tc * C;
  }
  float m = -INFINITY, s = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p0 = 0; p0 <= t; p0 += 4) {                                                 // uniform over the wavefront
    const int p = p0 + sub;
    const bool live = p <= t;
    float4 kk = k_new, vv = v_new;
    int64_t at = (int64_t)p * C;
    if (kBeam) at += to_event + (int64_t)__shfl(slot, p & 63, 64) * Tc * C;             // (every lane takes part in the shuffle)
    if (p < t) {                                                                       // (p == t: the registers; p > t: unused)
      kk = *reinterpret_cast<const float4 *>(kc + at);
      vv = *reinterpret_cast<const float4 *>(vc + at);
    }
    float d = fmaf(q.x, kk.x, fmaf(q.y, kk.y, fmaf(q.z, kk.z, q.w * kk.w)));
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);                         // over the 16 lanes of the position
    if (live) {
      const float sc = d * 0.125f;                                                     // 1 / sqrt(64)
      const float mn = fmaxf(m, sc);
      const float f = m == -INFINITY ? 0.f : expf(m - mn), w = expf(sc - mn);
      s = s * f + w;
      acc.x = fmaf(w, vv.x, acc.x * f); acc.y = fmaf(w, vv.y, acc.y * f);
      acc.z = fmaf(w, vv.z, acc.z * f); acc.w = fmaf(w, vv.w, acc.w * f);
      m = mn;
    }
  }
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {                                                 // the four quarter-waves
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    float4 a2;
    a2.x = __shfl_xor(acc.x, o, 64); a2.y = __shfl_xor(acc.y, o, 64);
    a2.z = __shfl_xor(acc.z, o, 64); a2.w = __shfl_xor(acc.w, o, 64);
    merge(m, s, acc, m2, s2, a2);
  }
  // residual (every quarter-wave holds the same context now; quarter 0 carries the row on)
  const float4 xr = *reinterpret_cast<const float4 *>(xres + (int64_t)row * ld_x + col);
  const float inv = 1.f / s;
  float4 y = make_float4(xr.x + acc.x * inv, xr.y + acc.y * inv, xr.z + acc.z * inv, xr.w + acc.w * inv);
  // norm1 over the C channels of the row: mean
  float part = sub == 0 ? (y.x + y.y) + (y.z + y.w) : 0.f;
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if (lane == 0) s_part[head] = part;
  __syncthreads();
  float mean = 0.f;
  for (int h = 0; h < H; ++h) mean += s_part[h];
  mean /= (float)C;
  y.x -= mean; y.y -= mean; y.z -= mean; y.w -= mean;
  float part2 = sub == 0 ? fmaf(y.x, y.x, y.y * y.y) + fmaf(y.z, y.z, y.w * y.w) : 0.f;
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) part2 += __shfl_xor(part2, o, 64);
  if (lane == 0) s_part2[head] = part2;
  __syncthreads();
  float var = 0.f;
  for (int h = 0; h < H; ++h) var += s_part2[h];
  const float rstd = 1.f / sqrtf(var / (float)C + eps);
  const float4 g = *reinterpret_cast<const float4 *>(gamma + col), b = *reinterpret_cast<const float4 *>(beta + col);
  const float4 o4 = make_float4(fmaf(y.x * rstd, g.x, b.x), fmaf(y.y * rstd, g.y, b.y), fmaf(y.z * rstd, g.z, b.z),
                                fmaf(y.w * rstd, g.w, b.w));
  if (sub == 0) *reinterpret_cast<float4 *>(out + (int64_t)row * C + col) = o4;
  if (amax_out) {
    float mx = fmaxf(fmaxf(fabsf(o4.x), fabsf(o4.y)), fmaxf(fabsf(o4.z), fabsf(o4.w)));
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) s_max[head] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int h = 1; h < H; ++h) mx = fmaxf(mx, s_max[h]);
      amax_out[row] = mx;
    }
  }
}

inline bool misaligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

extern "C" {

int gvl_capt_embed_f32(const float *embed, int n_vocab, const float *pos_table, int pos_rows, const int64_t *it, int t, int n,
                       int C, float *x, float *amax, void *stream) {
  if (n < 0 || n_vocab < 1 || pos_rows < 0 || t < 0 || C < 4 || (C & 3))
    return fail(GVL_EINVAL, "gvl_capt_embed_f32: bad sizes n=%d vocab=%d pos_rows=%d t=%d C=%d (C %% 4 == 0)", n, n_vocab, pos_rows,
                t, C);
  if (n == 0) return 0;
  if (!embed || !it || !x || !amax || (pos_rows > 0 && !pos_table)) return fail(GVL_EINVAL, "gvl_capt_embed_f32: null pointer");
  if (misaligned16(embed) || misaligned16(x) || (pos_table && misaligned16(pos_table)))
    return fail(GVL_EINVAL, "gvl_capt_embed_f32: embed, pos_table and x must be 16-byte aligned");
  return gvl::launch(GVL_PROF_CAPT_EMBED, n, t, "k_capt_embed", k_capt_embed, dim3(n), dim3(64), 0, (hipStream_t)stream, embed,
                     n_vocab, pos_table, pos_rows, it, t, C, x, amax);
}

int gvl_capt_attend_applicable(int H, int D, int positions) {
  return D == kHeadDim && H >= 1 && H <= kMaxHeads && positions >= 1 && positions <= kMaxPositions;
}

int gvl_capt_attend_f32(const float *qkv, int64_t ld_qkv, const float *x, int64_t ld_x, float *cache, int n, int positions, int t,
                        int H, const float *gamma, const float *beta, float eps, float *out, float *amax_out, void *stream) {
  if (!gvl_capt_attend_applicable(H, kHeadDim, positions))
    return fail(GVL_EINVAL, "gvl_capt_attend_f32: serves head dimension 64, 1 <= H <= %d, 1 <= positions <= %d (got H=%d positions=%d)",
                kMaxHeads, kMaxPositions, H, positions);
  const int C = H * kHeadDim;
  if (n < 0 || t < 0 || t >= positions || ld_qkv < 3 * C || (ld_qkv & 3) || ld_x < C || (ld_x & 3))
    return fail(GVL_EINVAL, "gvl_capt_attend_f32: bad sizes n=%d t=%d positions=%d ld_qkv=%lld ld_x=%lld (0 <= t < positions, "
                "row strides multiples of 4 that hold the row)", n, t, positions, (long long)ld_qkv, (long long)ld_x);
  if (n == 0) return 0;
  if (!qkv || !x || !cache || !gamma || !beta || !out) return fail(GVL_EINVAL, "gvl_capt_attend_f32: null pointer");
  if (misaligned16(qkv) || misaligned16(x) || misaligned16(cache) || misaligned16(gamma) || misaligned16(beta) || misaligned16(out))
    return fail(GVL_EINVAL, "gvl_capt_attend_f32: every tensor must be 16-byte aligned");
  return gvl::launch(GVL_PROF_CAPT_ATTEND, n, t, "k_capt_attend", k_capt_attend<false>, dim3(n), dim3(64 * H), 0,
                     (hipStream_t)stream, qkv, ld_qkv, x, ld_x, cache, (const unsigned char *)nullptr, 1, n, positions, t, H, gamma,
                     beta, eps, out, amax_out);
}

int gvl_capt_attend_beam_applicable(int H, int D, int positions, int W) {
  return gvl_capt_attend_applicable(H, D, positions) && W >= 1 && W <= kMaxBeam;
}

int gvl_capt_attend_beam_f32(const float *qkv, int64_t ld_qkv, const float *x, int64_t ld_x, float *cache,
                             const unsigned char *lineage, int n, int W, int positions, int t, int H, const float *gamma,
                             const float *beta, float eps, float *out, float *amax_out, void *stream) {
  if (!gvl_capt_attend_beam_applicable(H, kHeadDim, positions, W))
    return fail(GVL_EINVAL, "gvl_capt_attend_beam_f32: serves head dimension 64, 1 <= H <= %d, 1 <= positions <= %d, 1 <= W <= %d "
                "(got H=%d positions=%d W=%d)", kMaxHeads, kMaxPositions, kMaxBeam, H, positions, W);
  const int C = H * kHeadDim;
  if (n < 0 || (int64_t)n * W > 0x7fffffff || t < 0 || t >= positions || ld_qkv < 3 * C || (ld_qkv & 3) || ld_x < C || (ld_x & 3))
    return fail(GVL_EINVAL, "gvl_capt_attend_beam_f32: bad sizes n=%d W=%d t=%d positions=%d ld_qkv=%lld ld_x=%lld (0 <= t < "
                "positions, row strides multiples of 4 that hold the row)", n, W, t, positions, (long long)ld_qkv, (long long)ld_x);
  if (n == 0) return 0;
  if (!qkv || !x || !cache || !lineage || !gamma || !beta || !out) return fail(GVL_EINVAL, "gvl_capt_attend_beam_f32: null pointer");
  if (misaligned16(qkv) || misaligned16(x) || misaligned16(cache) || misaligned16(gamma) || misaligned16(beta) || misaligned16(out))
    return fail(GVL_EINVAL, "gvl_capt_attend_beam_f32: every fp32 tensor must be 16-byte aligned (the lineage bytes need not be)");
  const int rows = n * W;
  return gvl::launch(GVL_PROF_CAPT_ATTEND_BEAM, rows, t, "k_capt_attend_beam", k_capt_attend<true>, dim3(rows), dim3(64 * H), 0,
                     (hipStream_t)stream, qkv, ld_qkv, x, ld_x, cache, lineage, W, rows, positions, t, H, gamma, beta, eps, out,
                     amax_out);
}

}  // extern "C"
