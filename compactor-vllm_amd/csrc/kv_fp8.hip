// FP8 (OCP e4m3) paged KV cache for gfx950: quantising stores and the decode-attention kernel that reads them.
//
// Format: k_cache / v_cache [cache_rows, D] one e4m3 code per element, k_scale / v_scale
// [cache_rows] one fp32 scale per physical row.  For a row x[D]:
//     a = max(max_d |x_d|, 1e-30f);  scale = a / 448 (IEEE);  inv = 448 / a (IEEE);  code_d = rne_e4m3(x_d * inv)
// and the value read back is float(code) * scale.  |x * inv| <= 448, so the conversion never saturates.
//
// Stores: a row is D/16 lanes, each holding 16 source elements; the row maximum is a DPP all-reduce over those lanes,
// the lanes quantise from registers and write 16 B of codes each, the first lane writes the scale.  Addressing, slot
// order, the RESERVED-row rule and the length updates are those of store_kv.hip.
//
// Decode attention (decode_fp8_kernel): one workgroup of 4 waves per (b, kv-head, split) as in decode_attn.hip, and the
// same streaming skeleton - wave-private LDS rings filled by LDS-DMA, a counted vmcnt, no barrier in the loop, page ids
// windowed through registers - but the arithmetic is on the matrix cores:
//   * a unit = 32 consecutive rows: D/32 KiB of K codes, the same of V codes, and one 256 B DMA that brings the 32
//     k-scales (lanes 0-31) and the 32 v-scales (lanes 32-63).
//   * codes -> bf16 / f16 with v_cvt_scalef32_pk_{bf16,f16}_fp8 (scale 1.0: e4m3 is exact in both), a cost that does not
//     depend on G.
//   * S^T[row, head] = K . Q^T with v_mfma_f32_16x16x32: rows in M (two blocks of 16 per unit), the G query heads in N
//     (padded to 16 with zero columns), D/32 instructions per block.  The contraction index may be permuted freely as
//     long as both operands agree, so lane (row i, quarter g) simply reads the D/4 contiguous bytes g of row i and Q's
//     operand is laid out to match: no transposition on the K side.
//   * fp32 logits * k_scale[row] * sm_scale, online softmax in natural exp; head = lane % 16 both in the logits and in
//     the output accumulator, so the rescale factor never crosses lanes.  The only cross-lane step is the row maximum
//     over the four lane quarters (two permutes per 32 rows).
//   * O^T[d, head] += V^T . P^T: P * v_scale[row] goes straight from the logits' accumulator layout into the B operand
//     (lane quarter g holds rows 4g..4g+3 of both 16-row blocks, which DEFINES the order of the contraction index); V^T
//     comes out of LDS with ds_read_b64_tr_b8, whose 16 source lanes are pointed at exactly those rows.  P is fed as
//     hi + lo (two MFMAs per 16 dims) so that its 8/11-bit rounding does not enter the result: what is left is fp32
//     accumulation and the output rounding, as in the 16-bit kernel.  With f16, P * v_scale is carried times 2^9 (exact)
//     to stay clear of f16 subnormals.
//   * LDS image: the DMA's source addresses are permuted (16 B chunk c of row r lands at chunk c ^ swz(r)), free on the
//     global side and conflict-free for both the 16 B row reads of K and the transposing reads of V.
// Splits are merged by decode_stage2_kernel (decode_attn.hip) from normalised fp32 partials + LSE; one split writes
// the output directly.  No in-launch merge.  The shard form of a split-KV decode (cvllm_decode_attn_lse_fp8, and
// cvllm_decode_append_attn_lse_fp8 with the fused append below) also returns the LSE of the scaled logits per query head:
// with one split decode_fp8_kernel<.., LSE = true> writes M + log(den) from the state its output pass holds after the wave
// merge, otherwise decode_stage2_kernel writes it from the part_lse words.
//
// Fused append (decode_fp8_kernel<.., APPEND = true>, cvllm_decode_append_attn_fp8): the contract of the 16-bit fused
// append (decode_attn.hip).  The new token's row of (b, h) belongs at position L_old; every workgroup works with
// L = L_old + 1.  Row L_old lies in one 32-row unit of one split: the wave that owns that unit is the only one that
// touches the row.  Every wave quantises the new K row (lanes 0..D/16-1) and V row (lanes 8..8+D/16-1) up front with
// quant_row - ordinary loads, retired before the first LDS-DMA.  The owner lets the unit's DMA land (it fetched the
// slot's stale bytes), then patches the unit's LDS image with ds_write - D code bytes of K and of V at the swizzled
// chunk positions, the two scales in the scale block - and runs the unit through the unchanged MFMA path: bit-identical
// to store-then-attend.  As its last act it writes codes and scales to the paged cache with vector stores; no other
// workgroup reads that slot in this launch.  L_old + 1 is published by the workgroup itself with one split (after the
// barrier in front of the wave merge: every wave has read L_old) and by decode_stage2_kernel otherwise; stage 1 never
// writes a length when stage 2 follows.
#include "common.h"

namespace cvllm {

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x2_t __attribute__((ext_vector_type(2)));

template <int LPR>
__device__ __forceinline__ float group_allreduce_max(float v) {
  // all-reduce over the LPR (4 or 8) consecutive lanes that share one row
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true)));  // xor 1
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true)));  // xor 2
  if (LPR >= 8)
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true)));  // row_half_mirror
  return v;
}

// ---- the shared row writer -------------------------------------------------------------------------------------------
// Called together by the D/16 lanes of a row, which must be aligned inside a 16-lane DPP row; `src` = the lane's 16
// source elements.  quant_row leaves the lane's 16 B of codes in `c` and returns the row's scale (the same in every lane
// of the row); quant_row_store also writes them (`codes` = the lane's 16 B).
template <typename T, int D>
__device__ __forceinline__ float quant_row(const uint16_t* __restrict__ src, uint4& c) {
  constexpr int LPR = D / 16;
  const uint4 u0 = *reinterpret_cast<const uint4*>(src), u1 = *reinterpret_cast<const uint4*>(src + 8);
  const uint32_t w[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
  float x[16];
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float2 t = unpack2<T>(w[i]);
    x[2 * i] = t.x;
    x[2 * i + 1] = t.y;
    a = fmaxf(a, fmaxf(fabsf(t.x), fabsf(t.y)));
  }
  a = fmaxf(group_allreduce_max<LPR>(a), 1e-30f);
  const float scale = __fdiv_rn(a, 448.f);
  const float inv = __fdiv_rn(448.f, a);
  uint32_t cw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * i] * inv, x[4 * i + 1] * inv, 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * i + 2] * inv, x[4 * i + 3] * inv, p, true);
    cw[i] = (uint32_t)p;
  }
  c = make_uint4(cw[0], cw[1], cw[2], cw[3]);
  return scale;
}
template <typename T, int D>
__device__ __forceinline__ void quant_row_store(const uint16_t* __restrict__ src, uint8_t* __restrict__ codes,
                                                float* __restrict__ scale_dst, bool first_lane) {
  uint4 c;
  const float scale = quant_row<T, D>(src, c);
  *reinterpret_cast<uint4*>(codes) = c;
  if (first_lane) *scale_dst = scale;
}

__device__ __forceinline__ int find_seq_fp8(const int* __restrict__ cu, int B, int n) {
  int lo = 0, hi = B - 1;  // largest b with cu[b] <= n
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cu[mid] <= n) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- decode append ---------------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(256) void decode_store_fp8_kernel(
    const uint16_t* __restrict__ key, const uint16_t* __restrict__ value, int64_t sk_b, int64_t sk_h, int64_t sv_b,
    int64_t sv_h, const int* __restrict__ bmap, int* __restrict__ bh_lens, const int* __restrict__ page_table,
    uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, float* __restrict__ ksc, float* __restrict__ vsc, int BH, int HKV,
    int PS, int NLP, int reserved) {
  constexpr int LPR = D / 16;
  const int row = (blockIdx.x * 256 + threadIdx.x) / LPR;  // (b,h) pair; the lanes of a row leave together
  const int dl = threadIdx.x % LPR;
  if (row >= BH) return;
  const int b = row / HKV, h = row % HKV;
  const int bt = bmap[b];
  if (bt == reserved) return;
  const int L = bh_lens[row];
  const int pg = page_table[((size_t)bt * HKV + h) * NLP + L / PS];
  const size_t prow = (size_t)pg * PS + L % PS;
  quant_row_store<T, D>(key + b * sk_b + h * sk_h + dl * 16, kc + prow * D + dl * 16, ksc + prow, dl == 0);
  quant_row_store<T, D>(value + b * sv_b + h * sv_h + dl * 16, vc + prow * D + dl * 16, vsc + prow, dl == 0);
  if (dl == 0) bh_lens[row] = L + 1;  // every lane of the row read L above, in the same instruction stream
}

// ---- store every new row -----------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(256) void store_all_fp8_kernel(
    const uint16_t* __restrict__ key, const uint16_t* __restrict__ value, int64_t sk_n, int64_t sk_h, int64_t sv_n,
    int64_t sv_h, const int* __restrict__ cu, const int* __restrict__ bmap, const int* __restrict__ bh_lens,
    const int* __restrict__ page_table, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, float* __restrict__ ksc,
    float* __restrict__ vsc, int B, int N, int HKV, int PS, int NLP) {
  constexpr int LPR = D / 16;
  constexpr int RPB = 256 / LPR;
  const int dl = threadIdx.x % LPR;
  const int rl = threadIdx.x / LPR;
  const long total = (long)N * HKV;
  for (long r = (long)blockIdx.x * RPB + rl; r < total; r += (long)gridDim.x * RPB) {
    const int n = (int)(r / HKV), h = (int)(r % HKV);
    const int b = find_seq_fp8(cu, B, n);
    const int pos = bh_lens[b * HKV + h] + (n - cu[b]);
    const int pg = page_table[((size_t)bmap[b] * HKV + h) * NLP + pos / PS];
    const size_t prow = (size_t)pg * PS + pos % PS;
    quant_row_store<T, D>(key + (size_t)n * sk_n + h * sk_h + dl * 16, kc + prow * D + dl * 16, ksc + prow, dl == 0);
    quant_row_store<T, D>(value + (size_t)n * sv_n + h * sv_h + dl * 16, vc + prow * D + dl * 16, vsc + prow, dl == 0);
  }
}

__global__ void add_seq_lens_fp8_kernel(const int* __restrict__ cu, int* __restrict__ bh_lens, int B, int HKV) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * HKV) return;
  bh_lens[i] += cu[i / HKV + 1] - cu[i / HKV];
}

// ---- compaction from per-(b,h) kept-token lists (token order) ------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(256) void compact_store_fp8_kernel(
    const uint16_t* __restrict__ key, const uint16_t* __restrict__ value, int64_t sk_n, int64_t sk_h, int64_t sv_n,
    int64_t sv_h, const int* __restrict__ kept_idx, const int* __restrict__ new_lens, const int* __restrict__ cu,
    const int* __restrict__ bh_lens0, const int* __restrict__ page_table, const int* __restrict__ bmap,
    uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, float* __restrict__ ksc, float* __restrict__ vsc, int H,
    int max_seqlen, int PS, int NLP, int tiles_per_bh) {
  constexpr int LPR = D / 16;
  constexpr int RPB = 256 / LPR;
  const int bh = blockIdx.x / tiles_per_bh;
  const int tile = blockIdx.x % tiles_per_bh;
  const int b = bh / H, h = bh % H;
  const int L0 = bh_lens0[bh];
  const int cnt = new_lens[bh] - L0;
  const int dl = threadIdx.x % LPR;
  const int rl = threadIdx.x / LPR;
  const int* list = kept_idx + (size_t)bh * max_seqlen;
  const int* pt = page_table + ((size_t)bmap[b] * H + h) * NLP;
  const int n0 = cu[b];
  const int Lb1 = cu[b + 1] - n0 - 1;
  for (int j = tile * RPB + rl; j < cnt; j += tiles_per_bh * RPB) {
    const int n = n0 + max(0, min(list[j], Lb1));  // clamped into the sequence, as compact_store_kernel
    const int pos = L0 + j;
    const size_t prow = (size_t)pt[pos / PS] * PS + pos % PS;
    quant_row_store<T, D>(key + (size_t)n * sk_n + h * sk_h + dl * 16, kc + prow * D + dl * 16, ksc + prow, dl == 0);
    quant_row_store<T, D>(value + (size_t)n * sv_n + h * sv_h + dl * 16, vc + prow * D + dl * 16, vsc + prow, dl == 0);
  }
}

// ---- compaction IN PLACE (last chunk of a chunked prefill on an FP8 cache) --------------------------------------------------
// Sibling of compact_inplace_kernel (store_kv.hip): the kept rows of every (b,h) move down to slots dst_base.. in token
// order; a row's D bytes of codes and its two fp32 scales move together and nothing is re-quantised, so the result is
// what compact_store_fp8_kernel writes from the packed 16-bit rows, bit for bit.  The no-overlap argument is that
// kernel's: with an ascending kept list slot j receives the row of token t_j >= j, tile i writes slots below
// dst_base + TILE (i + 1) and every source of a later tile lies at or above src_base + TILE (i + 1); inside a tile a
// barrier separates all loads from all stores, and the next tile's loads are issued before this tile's stores.
// A row is D bytes here, not 2 D: D / 16 lanes of 16 B; every lane of a row carries the row's two scales, lane 0 writes them.
template <int D>
__global__ __launch_bounds__(256) void compact_inplace_fp8_kernel(
    const int* __restrict__ kept_idx, const int* __restrict__ new_lens, const int* __restrict__ dst_base,
    const int* __restrict__ src_base, const int* __restrict__ page_table, const int* __restrict__ bmap,
    uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, float* __restrict__ ksc, float* __restrict__ vsc, int H,
    int max_seqlen, int PS, int NLP) {
  constexpr int LPR = D / 16;         // lanes per row
  constexpr int RPP = 256 / LPR;      // rows per pass of the workgroup
  constexpr int TILE = 128;           // rows per tile, as the 16-bit kernel at D = 128
  constexpr int PASSES = TILE / RPP;  // rows per thread and tile
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int d0 = dst_base[bh], s0 = src_base[bh];
  const int cnt = new_lens[bh] - d0;
  const int tok_max = NLP * PS - 1 - s0;  // last row the page table can address
  const int dl = threadIdx.x % LPR, rl = threadIdx.x / LPR;
  const int* list = kept_idx + (size_t)bh * max_seqlen;
  const int* pt = page_table + ((size_t)bmap[b] * H + h) * NLP;
  auto row_of = [&](int pos) { return (size_t)pt[pos / PS] * PS + pos % PS; };
  struct Rows {
    uint4 k[PASSES], v[PASSES];
    float ks[PASSES], vs[PASSES];
  };
  Rows buf[2];
  auto load_tile = [&](int t0, Rows& x) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int j = t0 + p * RPP + rl;
      if (j < cnt) {
        const size_t a = row_of(s0 + max(0, min(list[j], tok_max)));  // clamped: see compact_store_kernel
        x.k[p] = *reinterpret_cast<const uint4*>(kc + a * D + dl * 16);
        x.v[p] = *reinterpret_cast<const uint4*>(vc + a * D + dl * 16);
        x.ks[p] = ksc[a];
        x.vs[p] = vsc[a];
      }
    }
  };
  auto store_tile = [&](int t0, const Rows& x) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int j = t0 + p * RPP + rl;
      if (j < cnt) {
        const size_t a = row_of(d0 + j);
        *reinterpret_cast<uint4*>(kc + a * D + dl * 16) = x.k[p];
        *reinterpret_cast<uint4*>(vc + a * D + dl * 16) = x.v[p];
        if (dl == 0) {
          ksc[a] = x.ks[p];
          vsc[a] = x.vs[p];
        }
      }
    }
  };
  if (cnt <= 0) return;
  load_tile(0, buf[0]);
  for (int t0 = 0; t0 < cnt; t0 += 2 * TILE) {
    if (t0 + TILE < cnt) load_tile(t0 + TILE, buf[1]);
    __syncthreads();  // every row of tile t0 is in registers (the barrier also drains each wave's loads)
    store_tile(t0, buf[0]);
    if (t0 + TILE >= cnt) break;
    if (t0 + 2 * TILE < cnt) load_tile(t0 + 2 * TILE, buf[0]);
    __syncthreads();
    store_tile(t0 + TILE, buf[1]);
  }
}

// ---- decode attention --------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Ring reads are inline asm with their own lgkmcnt wait: hipcc would otherwise drain vmcnt(0) in front of every LDS read
// while an LDS-DMA is pending, and the results must not be touched before the wait.
__device__ __forceinline__ void lds_read4_b128(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, u32x4_t& r0,
                                               u32x4_t& r1, u32x4_t& r2, u32x4_t& r3) {
  asm volatile(
      "ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3)
      : "memory");
}
__device__ __forceinline__ void lds_read2_b128(uint32_t a0, uint32_t a1, u32x4_t& r0, u32x4_t& r1) {
  asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(r0), "=&v"(r1)
               : "v"(a0), "v"(a1)
               : "memory");
}
// transposing read: inside a block of 16 lanes, lane t receives byte (t & 7) of the 8 bytes addressed by each of the
// lanes 2e + (t >> 3), e = 0..7
__device__ __forceinline__ void lds_read4_tr8(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, i32x2_t& r0,
                                              i32x2_t& r1, i32x2_t& r2, i32x2_t& r3) {
  asm volatile(
      "ds_read_b64_tr_b8 %0, %4\n\tds_read_b64_tr_b8 %1, %5\n\tds_read_b64_tr_b8 %2, %6\n\t"
      "ds_read_b64_tr_b8 %3, %7\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3)
      : "memory");
}

// two e4m3 codes (low or high half of w) -> one packed pair in the MFMA input type; exact
template <typename T, bool HI>
__device__ __forceinline__ uint32_t fp8x2_to16(uint32_t w);
template <>
__device__ __forceinline__ uint32_t fp8x2_to16<BF16, false>(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
}
template <>
__device__ __forceinline__ uint32_t fp8x2_to16<BF16, true>(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true));
}
template <>
__device__ __forceinline__ uint32_t fp8x2_to16<F16, false>(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false));
}
template <>
__device__ __forceinline__ uint32_t fp8x2_to16<F16, true>(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true));
}
template <typename T>
__device__ __forceinline__ s16x8 fp8x8_to16(uint32_t w0, uint32_t w1) {
  const u32x4_t r = {fp8x2_to16<T, false>(w0), fp8x2_to16<T, true>(w0), fp8x2_to16<T, false>(w1),
                     fp8x2_to16<T, true>(w1)};
  return __builtin_bit_cast(s16x8, r);
}

template <typename T>
__device__ __forceinline__ f32x4 mfma_16x16x32(s16x8 a, s16x8 b, f32x4 c);
template <>
__device__ __forceinline__ f32x4 mfma_16x16x32<BF16>(s16x8 a, s16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 mfma_16x16x32<F16>(s16x8 a, s16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

constexpr int F8_NW = 4;      // waves per workgroup
constexpr int F8_UR = 32;     // rows per unit
constexpr int F8_PGREGS = 8;  // page ids windowed through registers: 8 x 64 pages

template <int D, int R>
constexpr size_t fp8_ring_bytes() {
  return (size_t)F8_NW * R * (2 * F8_UR * D + 256);
}

// the appended row of the fused append; unused (and never read) without APPEND
struct Fp8NewRow {
  const uint16_t *key, *val;  // [B, HKV, D] in the model dtype
  int64_t sk_b, sk_h, sv_b, sv_h;
  int reserved;
};

// APPEND: seq_lens is the layer's full [Bmax+1, HKV] table indexed by bmap[b] (lengths BEFORE the append); otherwise the
// gathered [B, HKV] table.  The caches and scales are written with APPEND only.
// LSE: lse_out[B, HQ] also receives the natural-log LSE of the scaled logits over the rows this call saw (-inf for a
// (b, head) that saw none): one shard of a split-KV decode.  With one split this kernel writes it; otherwise
// decode_stage2_kernel does, from the part_lse words stage 1 writes anyway.  A compile-time flag, and lse_out is the
// LAST argument: the instantiations without it keep their instruction streams.
template <typename T, int D, int R, bool APPEND, bool LSE>
__global__ __launch_bounds__(F8_NW * 64) void decode_fp8_kernel(
    const uint16_t* __restrict__ q, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, float* __restrict__ ksc,
    float* __restrict__ vsc, int* __restrict__ seq_lens, const int* __restrict__ page_table,
    const int* __restrict__ bmap, uint16_t* __restrict__ out, float* __restrict__ part_o, float* __restrict__ part_lse,
    int HKV, int G, int PS, int NLP, int S, float scale, Fp8NewRow nr, float* __restrict__ lse_out) {
  constexpr int NW = F8_NW, UR = F8_UR;
  constexpr int CPR = D / 16;            // 16 B chunks per row
  constexpr int RPWIN = 256 / D;         // rows per 256 B of LDS (one pass over all banks)
  constexpr int NLK = UR * D / 1024;     // DMA instructions per K (and per V) of a unit
  constexpr int NKC = D / 32;            // MFMAs per 16-row block of logits
  constexpr int NDB = D / 16;            // 16-dim blocks of the output
  constexpr int KCH = CPR / 4;           // 16 B chunks of a row per lane quarter
  constexpr int KV_BYTES = UR * D;
  constexpr int UNIT_BYTES = 2 * KV_BYTES + 256;  // K codes | V codes | 32 k-scales | 32 v-scales
  constexpr int P = R - 1;               // units in flight ahead of the one being reduced
  constexpr int NDMA = 2 * NLK + 1;
  constexpr int NT_AUX = 2;              // non-temporal: the cache is read once per step
  constexpr float VF = (T::code == CVLLM_F16) ? 512.f : 1.f;  // P * v_scale is carried times VF (f16 subnormals)
  static_assert(NDMA * P <= 60, "vmcnt is a 6-bit counter");
  static_assert(D == 64 || D == 128, "head dim");

  extern __shared__ __attribute__((aligned(16))) char smem[];  // [NW][R][UNIT_BYTES]; a wave's ring is its staging area later

  const int bid = blockIdx.x;
  const int s = bid % S;
  const int bh = bid / S;
  const int h = bh % HKV;
  const int b = bh / HKV;
  const int HQ = HKV * G;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int j = lane & 15;  // row inside a 16-row block (A operand of the logits) = query head (everywhere else)
  const int g = lane >> 4;  // lane quarter

  const int bt = bmap[b];
  const int lidx = APPEND ? bt * HKV + h : bh;
  const int L_old = seq_lens[lidx];
  const bool append = APPEND && bt != nr.reserved;
  const int L = APPEND ? (append ? L_old + 1 : 0) : L_old;  // a reserved row attends to nothing and stores nothing
  // rows are dealt to the S splits in whole units, as decode_fused_kernel does
  const int U = (L + UR - 1) / UR;
  const int start = (int)(((long long)s * U) / S) * UR;
  const int end = min((int)(((long long)(s + 1) * U) / S) * UR, L);
  float* po = part_o + ((size_t)(b * S + s) * HQ + h * G) * D;
  float* pl = part_lse + (size_t)(b * S + s) * HQ + h * G;

  if (start >= end) {  // empty split (covers L == 0): zeros / a split that weighs nothing
    if (S == 1) {
      for (int i = tid; i < G * D; i += NW * 64) out[((size_t)b * HQ + h * G) * D + i] = 0;
      if constexpr (LSE)
        if (tid < G) lse_out[(size_t)b * HQ + h * G + tid] = -INFINITY;  // L == 0, or a RESERVED row of the fused append
    } else if (tid < G) {
      pl[tid] = -INFINITY;
    }
    return;
  }

  // Q as the B operand: lane (head j, quarter g) holds, for MFMA m, the 8 dims that K's lane (row, g) holds for it
  s16x8 qb[NKC];
#pragma unroll
  for (int m = 0; m < NKC; ++m) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);  // heads G..15: zero columns
    if (j < G)
      v = *reinterpret_cast<const uint4*>(q + ((size_t)b * HQ + h * G + j) * D + (g * KCH + m / 2) * 16 + (m % 2) * 8);
    qb[m] = __builtin_bit_cast(s16x8, v);
  }

  // Fused append.  Every wave quantises the new row, nothing diverges: in each 16-lane row lanes 0..CPR-1 take K and lanes
  // 8..8+CPR-1 take V, chunk nr_dl each (at D = 64 lanes 4-7 and 12-15 repeat them in DPP groups of their own).
  const int nr_v = (lane >> 3) & 1, nr_dl = lane & (CPR - 1);
  const bool nr_lane = lane < 16 && (lane & 7) < CPR;  // the lanes that write the row
  uint4 nr_codes = make_uint4(0u, 0u, 0u, 0u);
  float nr_scale = 0.f;
  int own_jw = -1;      // wave-local index of the unit that holds row L_old, in the one wave that owns it
  size_t own_prow = 0;  // the row's physical cache row, known when that unit is issued
  if constexpr (APPEND) {
    const uint16_t* src = nr_v ? nr.val + b * nr.sv_b + h * nr.sv_h : nr.key + b * nr.sk_b + h * nr.sk_h;
    nr_scale = quant_row<T, D>(src + nr_dl * 16, nr_codes);
    if (append && L_old >= start && L_old < end) {
      const int u = (L_old - start) / UR;
      if (u % NW == wave) own_jw = u / NW;
    }
    asm volatile("" : "+v"(nr_codes.x), "+v"(nr_codes.y), "+v"(nr_codes.z), "+v"(nr_codes.w), "+v"(nr_scale));
  }

  const int* pt = page_table + ((size_t)bt * HKV + h) * NLP;
  const int lp0 = start / PS;
  int pg_win = 0;  // first page of the register window, relative to lp0
  int pgreg[F8_PGREGS];
#pragma unroll
  for (int jj = 0; jj < F8_PGREGS; ++jj) {
    const int i = lp0 + lane + 64 * jj;
    pgreg[jj] = i < NLP ? pt[i] : 0;
  }
  // retire every ordinary load before the first LDS-DMA and hide the registers' origin (decode_fused_kernel)
#pragma unroll
  for (int jj = 0; jj < F8_PGREGS; ++jj) asm volatile("" : "+v"(pgreg[jj]));
#pragma unroll
  for (int m = 0; m < NKC; ++m) asm volatile("" : "+v"(qb[m]));

  // ---- per-lane constants of the LDS image ----------------------------------------------------------------------------
  // chunk c of row r of a unit lives at r*D + ((c ^ swz(r)) * 16), swz(r) = (r / RPWIN) % CPR
  int soff[NLK];  // global byte offset (inside the unit's contiguous run) this lane fetches with DMA instruction i
#pragma unroll
  for (int i = 0; i < NLK; ++i) {
    const int n = i * 64 + lane;  // 16 B slot the lane's data lands in
    const int r = n / CPR, p = n % CPR;
    soff[i] = r * D + ((p ^ ((r / RPWIN) & (CPR - 1))) * 16);
  }
  const float* scp = lane < 32 ? ksc + lane : vsc + (lane - 32);
  uint32_t kaddr[KCH];  // K: row j, chunks g*KCH + c2 (the second 16-row block is 16*D further: same swizzle)
#pragma unroll
  for (int c2 = 0; c2 < KCH; ++c2) kaddr[c2] = j * D + (((g * KCH + c2) ^ ((j / RPWIN) & (CPR - 1))) * 16);
  // V: source lane t = j of quarter g addresses row rk(g, t >> 1), bytes 8 * (t & 1) of the 16-dim block
  const int vrow = 4 * g + ((j >> 1) & 3) + 16 * (j >> 3);
  const uint32_t vbase = KV_BYTES + vrow * D + 8 * (j & 1);
  const uint32_t vsw = ((vrow / RPWIN) & (CPR - 1)) * 16;
  const uint32_t scoff = 2 * KV_BYTES + 16 * g;  // k-scales of rows 4g..4g+3; +64: second block; +128: v-scales

  const int nunits = (end - start + UR - 1) / UR;
  const int njw = nunits > wave ? (nunits - wave + NW - 1) / NW : 0;  // units owned by this wave
  char* ring = smem + wave * (R * UNIT_BYTES);
  const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)ring;

  auto page_of = [&](int lpi_rel) {
    const int lpi = lpi_rel - pg_win;
    int pg = __builtin_amdgcn_readlane(pgreg[0], lpi & 63);
#pragma unroll
    for (int jj = 1; jj < F8_PGREGS; ++jj)
      if ((lpi >> 6) == jj) pg = __builtin_amdgcn_readlane(pgreg[jj], lpi & 63);
    return pg;
  };

  auto issue = [&](int jw) {  // wave-local unit jw -> ring slot jw % R
    const int row0 = start + (wave + jw * NW) * UR;  // multiple of 32, PS % 32 == 0: the unit lies inside one page
    const int lpi_rel = row0 / PS - lp0;
    if (lpi_rel - pg_win >= 64 * F8_PGREGS) {  // rare: a split longer than 512 pages; the window only moves forward
      pg_win = lpi_rel;
#pragma unroll
      for (int jj = 0; jj < F8_PGREGS; ++jj) {
        const int i = lp0 + pg_win + lane + 64 * jj;
        pgreg[jj] = i < NLP ? pt[i] : 0;
      }
#pragma unroll
      for (int jj = 0; jj < F8_PGREGS; ++jj) asm volatile("" : "+v"(pgreg[jj]));
    }
    const size_t prow = (size_t)page_of(lpi_rel) * PS + row0 % PS;
    if constexpr (APPEND)
      if (jw == own_jw) own_prow = prow + (L_old - row0);  // kept: the page-id window may have moved on by then
    const uint8_t* kp = kc + prow * D;
    const uint8_t* vp = vc + prow * D;
    char* slot = ring + (jw % R) * UNIT_BYTES;
#pragma unroll
    for (int i = 0; i < NLK; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kp + soff[i]),
                                       (__attribute__((address_space(3))) void*)(slot + i * 1024), 16, 0, NT_AUX);
#pragma unroll
    for (int i = 0; i < NLK; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vp + soff[i]),
                                       (__attribute__((address_space(3))) void*)(slot + KV_BYTES + i * 1024), 16, 0,
                                       NT_AUX);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(scp + prow),
                                     (__attribute__((address_space(3))) void*)(slot + 2 * KV_BYTES), 4, 0, NT_AUX);
  };

  // online-softmax state of head j (m is the same in the four quarters, l is the quarter's partial sum) and
  // acc[db][r] = O[head j][16 db + 4 g + r]
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 acc[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int jw = 0; jw < P; ++jw)
    if (jw < njw) issue(jw);

  for (int jw = 0; jw < njw; ++jw) {
    if (jw + P < njw) {
      issue(jw + P);
      vm_wait<NDMA * P>();
    } else {
      vm_wait<0>();  // tail: drain
    }
    const uint32_t sl = ring_lds + (jw % R) * UNIT_BYTES;
    const int row0 = start + (wave + jw * NW) * UR;

    if constexpr (APPEND) {
      // The unit's DMA has landed (it fetched the new row's slot while that still held stale bytes): put the new row's
      // codes and scales over it, in front of the unit's first read.  LDS operations of a wave execute in order.
      if (jw == own_jw) {
        const int r = L_old - row0;
        const uint32_t ca = sl + nr_v * KV_BYTES + r * D + ((nr_dl ^ ((r / RPWIN) & (CPR - 1))) * 16);
        const uint32_t sa = sl + 2 * KV_BYTES + nr_v * 128 + 4 * r;
        if (nr_lane) {
          asm volatile("ds_write_b128 %0, %1" ::"v"(ca), "v"(__builtin_bit_cast(u32x4_t, nr_codes)) : "memory");
          if (nr_dl == 0) asm volatile("ds_write_b32 %0, %1" ::"v"(sa), "v"(nr_scale) : "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
    }

    // ---- logits of 2 x 16 rows ----------------------------------------------------------------------------------------
    u32x4_t kd[2][KCH], ks4[2], vs4[2];
    if constexpr (KCH == 2)
      lds_read4_b128(sl + kaddr[0], sl + kaddr[1], sl + kaddr[0] + 16 * D, sl + kaddr[1] + 16 * D, kd[0][0], kd[0][1],
                     kd[1][0], kd[1][1]);
    else
      lds_read2_b128(sl + kaddr[0], sl + kaddr[0] + 16 * D, kd[0][0], kd[1][0]);
    lds_read4_b128(sl + scoff, sl + scoff + 64, sl + scoff + 128, sl + scoff + 192, ks4[0], ks4[1], vs4[0], vs4[1]);
    f32x4 sacc[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      sacc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int mm = 0; mm < NKC; ++mm) {
        const u32x4_t kw = kd[rb][mm / 2];
        sacc[rb] = mfma_16x16x32<T>(fp8x8_to16<T>(kw[2 * (mm % 2)], kw[2 * (mm % 2) + 1]), qb[mm], sacc[rb]);
      }
    }
    // lane (head j, quarter g) now holds the logits of rows row0 + 16 rb + 4 g + r
    float sv[8];
    bool ok[8];
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int rb = e >> 2, r = e & 3;
      ok[e] = row0 + 16 * rb + 4 * g + r < end;
      sv[e] = ok[e] ? sacc[rb][r] * (__uint_as_float(ks4[rb][r]) * scale) : -INFINITY;
      mx = fmaxf(mx, sv[e]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // finite: the unit's first row is valid
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __expf(m_run - m_new);
    float pv[8];
    float psum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float p = __expf(sv[e] - m_new);
      psum += p;
      pv[e] = ok[e] ? p * (__uint_as_float(vs4[e >> 2][e & 3]) * VF) : 0.f;  // a select: stale scales may be anything
    }
    l_run = l_run * alpha + psum;
    m_run = m_new;
    // P^T as the B operand, hi + lo: contraction slot e of quarter g = row 16 (e >> 2) + 4 g + (e & 3)
    u32x4_t ph, plo;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      const uint32_t hi = pack2<T>(pv[e], pv[e + 1]);
      const float2 hf = unpack2<T>(hi);
      ph[e / 2] = hi;
      plo[e / 2] = pack2<T>(pv[e] - hf.x, pv[e + 1] - hf.y);
    }
    const s16x8 pbh = __builtin_bit_cast(s16x8, ph), pbl = __builtin_bit_cast(s16x8, plo);
    if (__any(alpha != 1.f)) {
#pragma unroll
      for (int db = 0; db < NDB; ++db) acc[db] *= alpha;
    }
    // rows past `end` (only in the split's last unit) hold stale codes - possibly NaN patterns: zero them (0 * NaN)
    uint32_t vm0 = 0xffffffffu, vm1 = 0xffffffffu;
    if (row0 + UR > end) {
      vm0 = (ok[0] ? 0xffu : 0u) | (ok[1] ? 0xff00u : 0u) | (ok[2] ? 0xff0000u : 0u) | (ok[3] ? 0xff000000u : 0u);
      vm1 = (ok[4] ? 0xffu : 0u) | (ok[5] ? 0xff00u : 0u) | (ok[6] ? 0xff0000u : 0u) | (ok[7] ? 0xff000000u : 0u);
    }
    // ---- O^T += V^T P^T -------------------------------------------------------------------------------------------------
#pragma unroll
    for (int d4 = 0; d4 < NDB; d4 += 4) {
      i32x2_t vt[4];
      lds_read4_tr8(sl + vbase + (((d4 + 0) * 16) ^ vsw), sl + vbase + (((d4 + 1) * 16) ^ vsw),
                    sl + vbase + (((d4 + 2) * 16) ^ vsw), sl + vbase + (((d4 + 3) * 16) ^ vsw), vt[0], vt[1], vt[2],
                    vt[3]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const s16x8 va = fp8x8_to16<T>((uint32_t)vt[i][0] & vm0, (uint32_t)vt[i][1] & vm1);
        acc[d4 + i] = mfma_16x16x32<T>(va, pbh, acc[d4 + i]);
        acc[d4 + i] = mfma_16x16x32<T>(va, pbl, acc[d4 + i]);
      }
    }
  }

  // ---- merge of the NW waves' states -----------------------------------------------------------------------------------
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  constexpr int ST_ML = 8 * D * 4;  // (m, l) pairs behind the fp32 numerators of up to 8 heads
  static_assert(ST_ML + 64 <= R * UNIT_BYTES, "staging area must fit the wave's ring");
  if (j < G) {  // all of this wave's DMA has landed and been read
#pragma unroll
    for (int db = 0; db < NDB; ++db)
      *reinterpret_cast<float4*>(ring + (j * D + 16 * db + 4 * g) * 4) =
          make_float4(acc[db][0], acc[db][1], acc[db][2], acc[db][3]);
    if (g == 0) *reinterpret_cast<float2*>(ring + ST_ML + j * 8) = make_float2(m_run, l_run);
  }
  __syncthreads();
  if constexpr (APPEND)
    if (S == 1 && tid == 0) seq_lens[lidx] = L_old + 1;  // one workgroup per (b, h); every wave read L_old before the barrier
  for (int idx = tid; idx < G * D; idx += NW * 64) {
    const int hd = idx / D, d = idx % D;
    float2 ml[NW];
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      ml[w] = *reinterpret_cast<const float2*>(smem + w * (R * UNIT_BYTES) + ST_ML + hd * 8);
      M = fmaxf(M, ml[w].x);  // finite: wave 0 owns the split's first unit
    }
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float a = __expf(ml[w].x - M);  // a wave without units: exp(-inf) = 0
      den = fmaf(a, ml[w].y, den);
      num = fmaf(a, *reinterpret_cast<const float*>(smem + w * (R * UNIT_BYTES) + (hd * D + d) * 4), num);
    }
    const float o = num / (den * VF);
    if (S == 1) {
      out[((size_t)b * HQ + h * G + hd) * D + d] = to16<T>(o);
      // (M, den) is head hd's state after the wave merge; the thread that owns the head's dim 0 writes M + log(den), the
      // value the branch below hands to stage 2 (den > 0: this split has at least one valid row)
      if constexpr (LSE)
        if (d == 0) lse_out[(size_t)b * HQ + h * G + hd] = den > 0.f ? M + __logf(den) : -INFINITY;
    } else {  // normalised fp32 partial + natural-log LSE: what decode_stage2_kernel reads
      po[hd * D + d] = o;
      if (d == 0) pl[hd] = M + __logf(den);
    }
  }
  if constexpr (APPEND) {
    // The owning wave writes the new row to the paged cache: last, so that nothing above waits for these stores.
    if (own_jw >= 0 && nr_lane) {
      *reinterpret_cast<uint4*>((nr_v ? vc : kc) + own_prow * D + nr_dl * 16) = nr_codes;
      if (nr_dl == 0) (nr_v ? vsc : ksc)[own_prow] = nr_scale;
    }
  }
}

// nr == nullptr: attention over the gathered lengths; otherwise the fused append on the layer's length table.
// lse_out != nullptr: the shard form (the LSE instantiation with one split, stage 2's LSE output otherwise)
template <typename T, int D>
static int launch_decode_fp8(const void* q, void* kc, void* vc, float* ksc, float* vsc, void* out, int* seq_lens,
                             const int* page_table, const int* bmap, char* ws, int B, int HQ, int HKV, int PS, int NLP,
                             float scale, int S, hipStream_t st, const Fp8NewRow* nr, float* lse_out) {
  constexpr int R = D == 128 ? 4 : 6;
  constexpr size_t smem = fp8_ring_bytes<D, R>();
  static_assert(smem <= 160 * 1024, "LDS budget");
  float* part_o = S > 1 ? reinterpret_cast<float*>(ws + DEC_WS_HEADER) : nullptr;
  float* part_lse = S > 1 ? part_o + (size_t)B * S * HQ * D : nullptr;
  auto launch = [&](auto kern, const Fp8NewRow& row) {
    set_dyn_lds_once(kern, (int)smem);
    hipLaunchKernelGGL(kern, dim3(B * HKV * S), dim3(F8_NW * 64), smem, st, (const uint16_t*)q, (uint8_t*)kc,
                       (uint8_t*)vc, ksc, vsc, seq_lens, page_table, bmap, (uint16_t*)out, part_o, part_lse, HKV,
                       HQ / HKV, PS, NLP, S, scale, row, lse_out);
  };
  const bool lse1 = lse_out != nullptr && S == 1;  // several splits: stage 1 is the plain kernel, stage 2 writes the LSE
  if (nr) {
    if (lse1) launch(decode_fp8_kernel<T, D, R, true, true>, *nr);
    else launch(decode_fp8_kernel<T, D, R, true, false>, *nr);
  } else {
    if (lse1) launch(decode_fp8_kernel<T, D, R, false, true>, Fp8NewRow{});
    else launch(decode_fp8_kernel<T, D, R, false, false>, Fp8NewRow{});
  }
  if (S > 1)  // with an appended row the merge kernel publishes L_old + 1: every stage-1 reader of L_old is done by then
    return launch_decode_stage2(part_o, part_lse, out, B, HQ, D, S, T::code, st, nr ? seq_lens : nullptr, bmap,
                                HQ / HKV, nr ? nr->reserved : -1, lse_out);
  return check_launch();
}

}  // namespace cvllm

using namespace cvllm;

#define DISPATCH_TD(DT_, D_, CALL)                                                     \
  if ((DT_) == CVLLM_F16) {                                                            \
    typedef F16 TT;                                                                    \
    if ((D_) == 64) { constexpr int DD = 64; CALL; }                                   \
    else if ((D_) == 128) { constexpr int DD = 128; CALL; }                            \
    else return CVLLM_ERR_SHAPE;                                                       \
  } else if ((DT_) == CVLLM_BF16) {                                                    \
    typedef BF16 TT;                                                                   \
    if ((D_) == 64) { constexpr int DD = 64; CALL; }                                   \
    else if ((D_) == 128) { constexpr int DD = 128; CALL; }                            \
    else return CVLLM_ERR_SHAPE;                                                       \
  } else return CVLLM_ERR_SHAPE;

extern "C" int cvllm_store_decode_kv_fp8(const void* key, const void* value, int64_t sk_b, int64_t sk_h, int64_t sv_b,
                                         int64_t sv_h, const int32_t* batch_mapping, int32_t* bh_lens,
                                         const int32_t* page_table, void* k_cache, void* v_cache, int B, int HKV, int D,
                                         int page_size, int n_logical_pages_max, int reserved_batch, int dtype,
                                         cvllm_stream_t stream, float* k_scale, float* v_scale) {
  if (!key || !value || !batch_mapping || !bh_lens || !page_table || !k_cache || !v_cache || !k_scale || !v_scale)
    return CVLLM_ERR_ARG;
  if (B <= 0 || HKV <= 0 || page_size <= 0 || n_logical_pages_max <= 0) return CVLLM_ERR_ARG;
  if ((sk_b % 8) || (sk_h % 8) || (sv_b % 8) || (sv_h % 8)) return CVLLM_ERR_SHAPE;  // 16 B source loads
  hipStream_t st = (hipStream_t)stream;
  const int BH = B * HKV;
  DISPATCH_TD(dtype, D, {
    const int rpb = 256 / (DD / 16);
    hipLaunchKernelGGL((decode_store_fp8_kernel<TT, DD>), dim3((BH + rpb - 1) / rpb), dim3(256), 0, st,
                       (const uint16_t*)key, (const uint16_t*)value, sk_b, sk_h, sv_b, sv_h, batch_mapping, bh_lens,
                       page_table, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale, v_scale, BH, HKV, page_size,
                       n_logical_pages_max, reserved_batch);
  });
  return check_launch();
}

extern "C" int cvllm_store_all_kv_fp8(const void* new_keys, const void* new_values, int64_t sk_n, int64_t sk_h,
                                      int64_t sv_n, int64_t sv_h, const int32_t* cu_seqlens_k,
                                      const int32_t* batch_mapping, int32_t* bh_lens, const int32_t* page_table,
                                      void* k_cache, void* v_cache, int B, int total_tokens, int HKV, int D,
                                      int page_size, int n_logical_pages_max, int dtype, cvllm_stream_t stream,
                                      float* k_scale, float* v_scale) {
  if (!new_keys || !new_values || !cu_seqlens_k || !batch_mapping || !bh_lens || !page_table || !k_cache || !v_cache ||
      !k_scale || !v_scale)
    return CVLLM_ERR_ARG;
  if (B <= 0 || HKV <= 0 || page_size <= 0 || n_logical_pages_max <= 0 || total_tokens < 0) return CVLLM_ERR_ARG;
  if ((sk_n % 8) || (sk_h % 8) || (sv_n % 8) || (sv_h % 8)) return CVLLM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (total_tokens > 0) {
    DISPATCH_TD(dtype, D, {
      const int rpb = 256 / (DD / 16);
      long blocks = ((long)total_tokens * HKV + rpb - 1) / rpb;
      if (blocks > 4096) blocks = 4096;  // grid-stride beyond 16 blocks per CU
      hipLaunchKernelGGL((store_all_fp8_kernel<TT, DD>), dim3((int)blocks), dim3(256), 0, st,
                         (const uint16_t*)new_keys, (const uint16_t*)new_values, sk_n, sk_h, sv_n, sv_h, cu_seqlens_k,
                         batch_mapping, bh_lens, page_table, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale, v_scale, B,
                         total_tokens, HKV, page_size, n_logical_pages_max);
    });
  } else if ((dtype != CVLLM_F16 && dtype != CVLLM_BF16) || (D != 64 && D != 128)) {
    return CVLLM_ERR_SHAPE;
  }
  hipLaunchKernelGGL(add_seq_lens_fp8_kernel, dim3((B * HKV + 255) / 256), dim3(256), 0, st, cu_seqlens_k, bh_lens, B,
                     HKV);
  return check_launch();
}

extern "C" int cvllm_compact_store_fp8(const void* new_keys, const void* new_vals, int64_t sk_n, int64_t sk_h,
                                       int64_t sv_n, int64_t sv_h, const int32_t* kept_idx, const int32_t* new_lens,
                                       const int32_t* cu_seqlens_k, const int32_t* bh_lens0, const int32_t* page_table,
                                       const int32_t* batch_mapping, void* k_cache, void* v_cache, int B, int H, int D,
                                       int max_seqlen, int page_size, int n_logical_pages_max, int dtype,
                                       cvllm_stream_t stream, float* k_scale, float* v_scale) {
  if (!new_keys || !new_vals || !kept_idx || !new_lens || !cu_seqlens_k || !bh_lens0 || !page_table || !batch_mapping ||
      !k_cache || !v_cache || !k_scale || !v_scale)
    return CVLLM_ERR_ARG;
  if (B <= 0 || H <= 0 || max_seqlen <= 0 || page_size <= 0 || n_logical_pages_max <= 0) return CVLLM_ERR_ARG;
  if ((sk_n % 8) || (sk_h % 8) || (sv_n % 8) || (sv_h % 8)) return CVLLM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_TD(dtype, D, {
    const int rpb = 256 / (DD / 16);
    int tiles = (max_seqlen + rpb * 8 - 1) / (rpb * 8);  // ~8 row-groups per block
    if (tiles < 1) tiles = 1;
    if (tiles > 256) tiles = 256;
    hipLaunchKernelGGL((compact_store_fp8_kernel<TT, DD>), dim3(B * H * tiles), dim3(256), 0, st,
                       (const uint16_t*)new_keys, (const uint16_t*)new_vals, sk_n, sk_h, sv_n, sv_h, kept_idx, new_lens,
                       cu_seqlens_k, bh_lens0, page_table, batch_mapping, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale,
                       v_scale, H, max_seqlen, page_size, n_logical_pages_max, tiles);
  });
  return check_launch();
}

extern "C" int cvllm_compact_cache_inplace_fp8(const int32_t* kept_idx, const int32_t* new_lens, const int32_t* dst_base,
                                              const int32_t* src_base, const int32_t* page_table,
                                              const int32_t* batch_mapping, void* k_cache, void* v_cache, int B, int H,
                                              int D, int max_seqlen, int page_size, int n_logical_pages_max,
                                              cvllm_stream_t stream, float* k_scale, float* v_scale) {
  if (!kept_idx || !new_lens || !dst_base || !src_base || !page_table || !batch_mapping || !k_cache || !v_cache ||
      !k_scale || !v_scale)
    return CVLLM_ERR_ARG;
  if (B <= 0 || H <= 0 || max_seqlen <= 0 || page_size <= 0 || n_logical_pages_max <= 0) return CVLLM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
#define CI_CALL(D_)                                                                                                  \
  hipLaunchKernelGGL((compact_inplace_fp8_kernel<D_>), dim3(B* H), dim3(256), 0, st, kept_idx, new_lens, dst_base,     \
                     src_base, page_table, batch_mapping, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale, v_scale, H, \
                     max_seqlen, page_size, n_logical_pages_max)
  if (D == 64) CI_CALL(64);
  else if (D == 128) CI_CALL(128);
  else return CVLLM_ERR_SHAPE;
#undef CI_CALL
  return check_launch();
}

// cvllm_decode_attn_fp8 (lse_out == nullptr) and cvllm_decode_attn_lse_fp8
static int decode_attn_fp8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale,
                           const float* v_scale, void* out, float* lse_out, const int32_t* seq_lens_bh,
                           const int32_t* page_table, const int32_t* batch_mapping, void* workspace,
                           size_t workspace_bytes, int B, int HQ, int HKV, int D, int page_size,
                           int n_logical_pages_max, float sm_scale, int n_splits, int dtype, cvllm_stream_t stream) {
  if (!q || !k_cache || !v_cache || !k_scale || !v_scale || !out || !seq_lens_bh || !page_table || !batch_mapping)
    return CVLLM_ERR_ARG;
  if (B <= 0 || HQ <= 0 || HKV <= 0 || n_splits <= 0 || n_logical_pages_max <= 0) return CVLLM_ERR_ARG;
  if (HQ % HKV != 0 || n_splits > 256) return CVLLM_ERR_SHAPE;
  const int G = HQ / HKV;
  if (G != 1 && G != 2 && G != 4 && G != 8) return CVLLM_ERR_SHAPE;
  if (page_size <= 0 || page_size % F8_UR != 0) return CVLLM_ERR_SHAPE;  // a unit of 32 rows must not straddle a page
  if (n_splits > 1 && (!workspace || workspace_bytes < cvllm_decode_workspace_bytes(B, HQ, D, n_splits)))
    return CVLLM_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_TD(dtype, D, {
    // without an appended row the kernel only reads the caches, the scales and the lengths
    return (launch_decode_fp8<TT, DD>(q, (void*)k_cache, (void*)v_cache, (float*)k_scale, (float*)v_scale, out,
                                      (int*)seq_lens_bh, page_table, batch_mapping, (char*)workspace, B, HQ, HKV,
                                      page_size, n_logical_pages_max, sm_scale, n_splits, st, nullptr, lse_out));
  });
  return CVLLM_ERR_SHAPE;
}

extern "C" int cvllm_decode_attn_fp8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale,
                                     const float* v_scale, void* out, const int32_t* seq_lens_bh,
                                     const int32_t* page_table, const int32_t* batch_mapping, void* workspace,
                                     size_t workspace_bytes, int B, int HQ, int HKV, int D, int page_size,
                                     int n_logical_pages_max, float sm_scale, int n_splits, int dtype,
                                     cvllm_stream_t stream) {
  return decode_attn_fp8(q, k_cache, v_cache, k_scale, v_scale, out, nullptr, seq_lens_bh, page_table, batch_mapping,
                         workspace, workspace_bytes, B, HQ, HKV, D, page_size, n_logical_pages_max, sm_scale, n_splits,
                         dtype, stream);
}

// One shard of a split-KV decode on an FP8 cache: cvllm_decode_attn_fp8 plus lse_out[B, HQ], the natural-log LSE of the
// scaled logits sm_scale * k_scale[row] * (q . code_row) over the rows this call saw (-inf when it saw none)
extern "C" int cvllm_decode_attn_lse_fp8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale,
                                         const float* v_scale, void* out, float* lse_out, const int32_t* seq_lens_bh,
                                         const int32_t* page_table, const int32_t* batch_mapping, void* workspace,
                                         size_t workspace_bytes, int B, int HQ, int HKV, int D, int page_size,
                                         int n_logical_pages_max, float sm_scale, int n_splits, int dtype,
                                         cvllm_stream_t stream) {
  if (!lse_out) return CVLLM_ERR_ARG;
  return decode_attn_fp8(q, k_cache, v_cache, k_scale, v_scale, out, lse_out, seq_lens_bh, page_table, batch_mapping,
                         workspace, workspace_bytes, B, HQ, HKV, D, page_size, n_logical_pages_max, sm_scale, n_splits,
                         dtype, stream);
}

// cvllm_decode_append_attn_fp8 (lse_out == nullptr) and cvllm_decode_append_attn_lse_fp8
static int decode_append_attn_fp8(const void* q, const void* key, const void* value, int64_t sk_b, int64_t sk_h,
                                  int64_t sv_b, int64_t sv_h, void* k_cache, void* v_cache, void* out, float* lse_out,
                                  int32_t* bh_seq_lens, const int32_t* page_table, const int32_t* batch_mapping,
                                  void* workspace, size_t workspace_bytes, int B, int HQ, int HKV, int D, int page_size,
                                  int n_logical_pages_max, float sm_scale, int n_splits, int reserved_batch, int dtype,
                                  cvllm_stream_t stream, float* k_scale, float* v_scale) {
  if (!q || !key || !value || !k_cache || !v_cache || !out || !bh_seq_lens || !page_table || !batch_mapping ||
      !k_scale || !v_scale)
    return CVLLM_ERR_ARG;
  if (B <= 0 || HQ <= 0 || HKV <= 0 || n_splits <= 0 || n_logical_pages_max <= 0) return CVLLM_ERR_ARG;
  if (HQ % HKV != 0 || n_splits > 256) return CVLLM_ERR_SHAPE;
  const int G = HQ / HKV;
  if (G != 1 && G != 2 && G != 4 && G != 8) return CVLLM_ERR_SHAPE;
  if (page_size <= 0 || page_size % F8_UR != 0) return CVLLM_ERR_SHAPE;
  if ((sk_b % 8) || (sk_h % 8) || (sv_b % 8) || (sv_h % 8)) return CVLLM_ERR_SHAPE;  // 16 B source loads
  if (n_splits > 1 && (!workspace || workspace_bytes < cvllm_decode_workspace_bytes(B, HQ, D, n_splits)))
    return CVLLM_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const Fp8NewRow nr{(const uint16_t*)key, (const uint16_t*)value, sk_b, sk_h, sv_b, sv_h, reserved_batch};
  DISPATCH_TD(dtype, D, {
    return (launch_decode_fp8<TT, DD>(q, k_cache, v_cache, k_scale, v_scale, out, bh_seq_lens, page_table,
                                      batch_mapping, (char*)workspace, B, HQ, HKV, page_size, n_logical_pages_max,
                                      sm_scale, n_splits, st, &nr, lse_out));
  });
  return CVLLM_ERR_SHAPE;
}

// The fused decode step on an FP8 cache: quantise and append the new K/V row of every (b,h) at
// bh_seq_lens[batch_mapping[b], h] (RESERVED rows skipped), attend over the rows including it, publish the new lengths.
extern "C" int cvllm_decode_append_attn_fp8(const void* q, const void* key, const void* value, int64_t sk_b,
                                            int64_t sk_h, int64_t sv_b, int64_t sv_h, void* k_cache, void* v_cache,
                                            void* out, int32_t* bh_seq_lens, const int32_t* page_table,
                                            const int32_t* batch_mapping, void* workspace, size_t workspace_bytes,
                                            int B, int HQ, int HKV, int D, int page_size, int n_logical_pages_max,
                                            float sm_scale, int n_splits, int reserved_batch, int dtype,
                                            cvllm_stream_t stream, float* k_scale, float* v_scale) {
  return decode_append_attn_fp8(q, key, value, sk_b, sk_h, sv_b, sv_h, k_cache, v_cache, out, nullptr, bh_seq_lens,
                                page_table, batch_mapping, workspace, workspace_bytes, B, HQ, HKV, D, page_size,
                                n_logical_pages_max, sm_scale, n_splits, reserved_batch, dtype, stream, k_scale,
                                v_scale);
}

// The append rank's step of a split-KV decode on an FP8 cache: the fused step above plus lse_out[B, HQ] over the rows
// INCLUDING the appended one (the owner wave patches it into the unit's LDS image before the unit is reduced); -inf on a
// RESERVED row, which attends to nothing
extern "C" int cvllm_decode_append_attn_lse_fp8(const void* q, const void* key, const void* value, int64_t sk_b,
                                                int64_t sk_h, int64_t sv_b, int64_t sv_h, void* k_cache,
                                                void* v_cache, void* out, float* lse_out, int32_t* bh_seq_lens,
                                                const int32_t* page_table, const int32_t* batch_mapping,
                                                void* workspace, size_t workspace_bytes, int B, int HQ, int HKV, int D,
                                                int page_size, int n_logical_pages_max, float sm_scale, int n_splits,
                                                int reserved_batch, int dtype, cvllm_stream_t stream, float* k_scale,
                                                float* v_scale) {
  if (!lse_out) return CVLLM_ERR_ARG;
  return decode_append_attn_fp8(q, key, value, sk_b, sk_h, sv_b, sv_h, k_cache, v_cache, out, lse_out, bh_seq_lens,
                                page_table, batch_mapping, workspace, workspace_bytes, B, HQ, HKV, D, page_size,
                                n_logical_pages_max, sm_scale, n_splits, reserved_batch, dtype, stream, k_scale,
                                v_scale);
}
