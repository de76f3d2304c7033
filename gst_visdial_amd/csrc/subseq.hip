// Substitution of wordpiece id sequences inside one utterance of a context row, on token ids (the coreference attack's
// substitute_word, utils/text_attack.py:93-100, restated without decode / str.replace / tokenize; the rule is stated with
// gstvd_subseq_replace_t in include/gstvd_hip.h).  One workgroup per row, the row in LDS; a row's substitutions are applied one
// after the other, each to the result of the one before.  Per substitution: a block scan of the separator flags finds the
// utterance, every position tests the match in parallel, one thread walks the utterance to pick the greedy non-overlapping
// matches (the only sequential part: at most one utterance's tokens), a block scan of the tokens each position emits gives every
// token its place, and the next row is written once.  No atomics, no workspace; every output element is written once.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_T = 1024;
constexpr int MAX_L = 16;

// Inclusive scan of a[0..T) (filled, behind a barrier) with b as the second buffer; returns the buffer that holds the result.
DEVFN int* block_scan(int* a, int* b, int T) {
  for (int off = 1; off < T; off <<= 1) {
    for (int p = threadIdx.x; p < T; p += NT) b[p] = a[p] + (p >= off ? a[p - off] : 0);
    __syncthreads();
    int* t = a; a = b; b = t;
  }
  return a;
}

__global__ __launch_bounds__(NT) void subseq_replace_kernel(gstvd_subseq_replace_t p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int T = p.T, tid = threadIdx.x, row = blockIdx.x;
  int64_t* cur = (int64_t*)smem;          // [T]
  int64_t* nxt = cur + T;                 // [T]
  int64_t* pa = nxt + T;                  // [16] the sequence looked for
  int64_t* pb = pa + MAX_L;               // [16] its replacement
  int* sa = (int*)(pb + MAX_L);           // [T] scan buffers
  int* sb = sa + T;
  int* emit = sb + T;                     // [T] tokens a position sends to the next row: 1, 0 inside a match, Lb at its start
  int* misc = emit + T;                   // lo, hi, matches so far, -
  uint8_t* mt = (uint8_t*)(misc + 4);     // [T] a matches here
  uint8_t* sel = mt + T;                  // [T] a chosen match starts here
  auto is_cont = [&](int64_t x) { return p.cont && x >= 0 && x < p.n_vocab && p.cont[x] != 0; };

  for (int q = tid; q < T; q += NT) cur[q] = p.ids[(int64_t)row * p.ld_ids + q];
  if (tid == 0) misc[2] = 0;
  int s0 = p.row_ptr[row], s1 = p.row_ptr[row + 1];
  s0 = s0 < 0 ? 0 : (s0 > p.n_subs ? p.n_subs : s0);
  s1 = s1 < s0 ? s0 : (s1 > p.n_subs ? p.n_subs : s1);
  __syncthreads();

  for (int si = s0; si < s1; ++si) {      // (everything that decides a `continue` is the same in all threads)
    const int u = p.subs[4 * si], off = p.subs[4 * si + 1], La = p.subs[4 * si + 2], Lb = p.subs[4 * si + 3];
    if (u < 0 || La < 1 || La > MAX_L || Lb < 1 || Lb > MAX_L || off < 0 || (int64_t)off + La + Lb > p.n_pieces) continue;
    if (tid < La) pa[tid] = p.pieces[off + tid];
    if (tid >= 32 && tid < 32 + Lb) pb[tid - 32] = p.pieces[off + La + tid - 32];
    for (int q = tid; q < T; q += NT) { sa[q] = cur[q] == p.sep; emit[q] = 1; sel[q] = 0; mt[q] = 0; }
    if (tid == 0) { misc[0] = u == 0 ? 1 : -1; misc[1] = -1; }
    __syncthreads();
    const int* cs = block_scan(sa, sb, T);
    for (int q = tid; q < T; q += NT)
      if (cur[q] == p.sep) {              // the u-th separator ends utterance u - 1, the (u + 1)-th ends utterance u
        if (cs[q] == u) misc[0] = q + 1;
        if (cs[q] == u + 1) misc[1] = q;
      }
    __syncthreads();
    const int lo = misc[0], hi = misc[1];
    __syncthreads();
    if (hi < 0) continue;                 // fewer than u + 1 separators: nothing to do
    for (int q = lo + tid; q < hi; q += NT) {
      bool ok = q + La <= hi;
      for (int k = 0; ok && k < La; ++k) ok = cur[q + k] == pa[k];
      if (ok && p.cont) ok = !is_cont(cur[q]) && (q + La == hi || !is_cont(cur[q + La]));
      mt[q] = ok;
    }
    __syncthreads();
    if (tid == 0) {                       // left to right, greedy, non-overlapping
      int c = 0;
      for (int q = lo; q < hi;) {
        if (mt[q]) {
          sel[q] = 1; emit[q] = Lb;
          for (int k = 1; k < La; ++k) emit[q + k] = 0;
          q += La; ++c;
        } else {
          ++q;
        }
      }
      misc[2] += c;
    }
    __syncthreads();
    for (int q = tid; q < T; q += NT) sa[q] = emit[q];
    __syncthreads();
    cs = block_scan(sa, sb, T);
    for (int q = tid; q < T; q += NT) {
      const int o = cs[q] - emit[q];
      if (sel[q]) {
        for (int k = 0; k < Lb; ++k)
          if (o + k < T) nxt[o + k] = pb[k];
      } else if (emit[q] && o < T) {
        nxt[o] = cur[q];
      }
    }
    for (int o = cs[T - 1] + tid; o < T; o += NT) nxt[o] = p.pad;      // tokens pushed past T are dropped, a shorter row is padded
    __syncthreads();
    int64_t* t = cur; cur = nxt; nxt = t;
  }

  for (int q = tid; q < T; q += NT) p.out_ids[(int64_t)row * p.ld_out + q] = cur[q];
  if (tid == 0) p.n_replaced[row] = misc[2];
  if (!p.segments && !p.sep_indices && !p.att_mask) return;
  for (int q = tid; q < T; q += NT) sa[q] = cur[q] == p.sep;
  __syncthreads();
  const int* cs = block_scan(sa, sb, T);
  const int64_t start = p.start_seg ? p.start_seg[(int64_t)row * p.ld_start] : 0;
  for (int q = tid; q < T; q += NT) {
    const int64_t x = cur[q];
    const int before = cs[q] - (x == p.sep);      // separators in front of q: a [SEP] still carries its utterance's segment
    if (p.segments) p.segments[(int64_t)row * p.ld_seg + q] = x == p.pad ? 0 : (start ^ (before & 1));
    if (p.att_mask) p.att_mask[(int64_t)row * p.ld_att + q] = x != p.pad ? 1.f : 0.f;
    if (p.sep_indices && x == p.sep && before < p.max_sep) p.sep_indices[(int64_t)row * p.ld_sep + before] = q;
  }
  if (p.sep_indices)
    for (int k = cs[T - 1] + tid; k < p.max_sep; k += NT) p.sep_indices[(int64_t)row * p.ld_sep + k] = 0;
}

}  // namespace

extern "C" int gstvd_subseq_replace(const gstvd_subseq_replace_t* a, gstvd_stream_t s) {
  if (!a || !a->ids || !a->out_ids || !a->n_replaced || !a->row_ptr) return GSTVD_E_NULL;
  if (a->n_subs > 0 && (!a->subs || !a->pieces)) return GSTVD_E_NULL;
  if (a->n < 1 || a->T < 1 || a->ld_ids < a->T || a->ld_out < a->T || a->n_subs < 0 || a->n_pieces < 0) return GSTVD_E_SHAPE;
  if (a->ids == a->out_ids) return GSTVD_E_SHAPE;                      // the input row is read, never written
  if (a->cont && a->n_vocab < 1) return GSTVD_E_SHAPE;
  if (a->segments && a->ld_seg < a->T) return GSTVD_E_SHAPE;
  if (a->att_mask && a->ld_att < a->T) return GSTVD_E_SHAPE;
  if (a->sep_indices && (a->max_sep < 1 || a->ld_sep < a->max_sep)) return GSTVD_E_SHAPE;
  if (a->T > MAX_T) return GSTVD_E_UNSUPPORTED;
  const int T = a->T;
  const int lds = 2 * T * (int)sizeof(int64_t) + 2 * MAX_L * (int)sizeof(int64_t) + (3 * T + 4) * (int)sizeof(int) + 2 * T;
  hipLaunchKernelGGL(subseq_replace_kernel, dim3((unsigned)a->n), dim3(NT), lds, (hipStream_t)s, *a);
  GSTVD_LAUNCH_CHECK();
  return 0;
}
