// MXFP4 (OCP e2m1 codes + one e8m0 power-of-two scale per 32 elements) paged KV cache for gfx950: quantising stores and
// the decode-attention kernel that reads them.
//
// Format: k_cache / v_cache [cache_rows, D/2] bytes, byte i of a row = element 2i in the low
// nibble and element 2i+1 in the high nibble; k_scale / v_scale [cache_rows, D/32] bytes.  For a block of 32 consecutive
// elements of a row:
//     a = max |x_d|;  f = exponent field of a as fp32;  s = max(f - 2, 0);  E = s - 127
//     code_d = e2m1(x_d * 2^-E), round to nearest, ties to the even code, saturating at +-6
// and the value read back is fp32(code) * 2^E.  The codes are computed with compares against the seven midpoints: the
// rule governs, not a conversion instruction.
//
// Stores: a row is D/16 lanes, each holding 16 source elements; a block is a pair of adjacent lanes, its maximum one DPP
// exchange inside the pair.  A lane packs its 16 codes into 8 bytes in registers and writes them with one 8 B store; the
// even lane of a pair writes the block's scale byte.  Addressing, slot order, the RESERVED-row rule and the length
// updates are those of store_kv.hip / kv_fp8.hip.  The in-place compaction behind a chunked prefill moves code and scale
// bytes as they are (compact_inplace_mxfp4_kernel); the prefill kernel that reads them is prefill_mxfp4.hip.
//
// Decode attention (decode_mxfp4_kernel): the streaming skeleton of decode_fp8_kernel - one workgroup of 4 waves per
// (b, kv-head, split), wave-private LDS rings filled by LDS-DMA, a counted vmcnt, no barrier in the loop, page ids
// windowed through registers - with a data path of its own:
//   * a unit = 32 consecutive rows: 16 D bytes of K codes, the same of V codes, and ONE 256 B DMA that brings the
//     unit's K scale bytes (lanes 0-31) and V scale bytes (lanes 32-63).  A unit is about half an FP8 unit, so the rings
//     are twice as deep (8 slots at D = 128, 12 at D = 64) to keep the same bytes in flight.
//   * codes -> bf16 / f16 with v_cvt_scalef32_pk_{bf16,f16}_fp4, the block's 2^E (exponent field = the scale byte) as the
//     scale operand: the scale folds in exactly and no multiply by a scale is left anywhere else.
//   * S^T[row, head] = K . Q^T with v_mfma_f32_16x16x32: rows in M, the G heads in N (padded to 16).  Lane (row i,
//     quarter g) reads the D/8 contiguous bytes g of row i - at D = 128 exactly scale block g, at D = 64 half of block
//     g / 2 - so a lane needs ONE K scale per 16-row block, and Q's operand is laid out to match.
//   * O^T[d, head] += V^T . P^T: ds_read_b64_tr_b8 transposes BYTES, i.e. pairs of codes: lane t of a 16-lane block
//     receives byte t of a 16 B chunk (dims 32 c + 2 t and 32 c + 2 t + 1) for the eight rows of its lane quarter.  Eight
//     conversions (one scale each: a chunk is one scale block) give eight (even, odd) pairs; their low halves form the A
//     operand of the even dims and their high halves that of the odd dims.  The accumulator of chunk c therefore holds
//     dims 32 c + 2 (4 g + r) + parity, which the epilogue writes back in natural order.  P is fed as hi + lo.
//   * LDS image: 16 B chunk c of row r lands at chunk c ^ swz(r) (the DMA's source addresses are permuted); swz is
//     chosen so that the K row reads and the transposing V reads each cover all banks once per pass.
//   * rows past the split's end may be stale: their logits / P are selected to -inf / 0, and their V codes AND scale
//     bytes are masked to zero before conversion (a stale scale byte of 255 is a NaN).
// Splits are merged by decode_stage2_kernel (decode_attn.hip); one split writes the output directly.
#include <type_traits>

#include "common.h"

namespace cvllm {

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef int i32x2_t __attribute__((ext_vector_type(2)));

// ---- the shared row writer -------------------------------------------------------------------------------------------
// Called together by the D/16 lanes of a row (lane dl holds elements 16 dl .. 16 dl + 15; lanes 2k, 2k+1 own block k and
// are DPP neighbours).  Leaves the lane's 16 codes in `c` and returns the block's scale byte.
template <typename T>
__device__ __forceinline__ uint32_t mx_quant16(const uint16_t* __restrict__ src, uint2& c) {
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
  a = fmaxf(a, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a), 0xB1, 0xf, 0xf, true)));  // xor 1
  const uint32_t f = (__float_as_uint(a) >> 23) & 0xffu;
  const uint32_t s = f > 2u ? f - 2u : 0u;
  const float inv = __uint_as_float((254u - s) << 23);  // 2^(127 - s) = 2^-E, a normal fp32 for every s <= 252
  uint32_t cw[2] = {0u, 0u};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float y = fabsf(x[i]) * inv;  // exact: a power of two, |y| < 8
    // the seven midpoints; a tie goes to the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4)
    uint32_t code = (uint32_t)(y > 0.25f) + (uint32_t)(y >= 0.75f) + (uint32_t)(y > 1.25f) + (uint32_t)(y >= 1.75f) +
                    (uint32_t)(y > 2.5f) + (uint32_t)(y >= 3.5f) + (uint32_t)(y > 5.f);
    code |= (__float_as_uint(x[i]) >> 28) & 8u;
    cw[i / 8] |= code << (4 * (i % 8));
  }
  c = make_uint2(cw[0], cw[1]);
  return s;
}
// `src` = the row's first source element; `codes` / `scales` = the row's D/2 code bytes and D/32 scale bytes
template <typename T, int D>
__device__ __forceinline__ void mx_row_store(const uint16_t* __restrict__ src, uint8_t* __restrict__ codes,
                                             uint8_t* __restrict__ scales, int dl) {
  uint2 c;
  const uint32_t s = mx_quant16<T>(src + dl * 16, c);
  *reinterpret_cast<uint2*>(codes + dl * 8) = c;
  if ((dl & 1) == 0) scales[dl >> 1] = (uint8_t)s;
}

__device__ __forceinline__ int find_seq_mx(const int* __restrict__ cu, int B, int n) {
  int lo = 0, hi = B - 1;  // largest b with cu[b] <= n
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cu[mid] <= n) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- decode append ---------------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(256) void decode_store_mxfp4_kernel(
    const uint16_t* __restrict__ key, const uint16_t* __restrict__ value, int64_t sk_b, int64_t sk_h, int64_t sv_b,
    int64_t sv_h, const int* __restrict__ bmap, int* __restrict__ bh_lens, const int* __restrict__ page_table,
    uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, uint8_t* __restrict__ ksc, uint8_t* __restrict__ vsc, int BH,
    int HKV, int PS, int NLP, int reserved) {
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
  mx_row_store<T, D>(key + b * sk_b + h * sk_h, kc + prow * (D / 2), ksc + prow * (D / 32), dl);
  mx_row_store<T, D>(value + b * sv_b + h * sv_h, vc + prow * (D / 2), vsc + prow * (D / 32), dl);
  if (dl == 0) bh_lens[row] = L + 1;  // every lane of the row read L above, in the same instruction stream
}

// ---- store every new row -----------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(256) void store_all_mxfp4_kernel(
    const uint16_t* __restrict__ key, const uint16_t* __restrict__ value, int64_t sk_n, int64_t sk_h, int64_t sv_n,
    int64_t sv_h, const int* __restrict__ cu, const int* __restrict__ bmap, const int* __restrict__ bh_lens,
    const int* __restrict__ page_table, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, uint8_t* __restrict__ ksc,
    uint8_t* __restrict__ vsc, int B, int N, int HKV, int PS, int NLP) {
  constexpr int LPR = D / 16;
  constexpr int RPB = 256 / LPR;
  const int dl = threadIdx.x % LPR;
  const int rl = threadIdx.x / LPR;
  const long total = (long)N * HKV;
  for (long r = (long)blockIdx.x * RPB + rl; r < total; r += (long)gridDim.x * RPB) {
    const int n = (int)(r / HKV), h = (int)(r % HKV);
    const int b = find_seq_mx(cu, B, n);
    const int pos = bh_lens[b * HKV + h] + (n - cu[b]);
    const int pg = page_table[((size_t)bmap[b] * HKV + h) * NLP + pos / PS];
    const size_t prow = (size_t)pg * PS + pos % PS;
    mx_row_store<T, D>(key + (size_t)n * sk_n + h * sk_h, kc + prow * (D / 2), ksc + prow * (D / 32), dl);
    mx_row_store<T, D>(value + (size_t)n * sv_n + h * sv_h, vc + prow * (D / 2), vsc + prow * (D / 32), dl);
  }
}

__global__ void add_seq_lens_mxfp4_kernel(const int* __restrict__ cu, int* __restrict__ bh_lens, int B, int HKV) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * HKV) return;
  bh_lens[i] += cu[i / HKV + 1] - cu[i / HKV];
}

// ---- compaction from per-(b,h) kept-token lists (token order) ------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(256) void compact_store_mxfp4_kernel(
    const uint16_t* __restrict__ key, const uint16_t* __restrict__ value, int64_t sk_n, int64_t sk_h, int64_t sv_n,
    int64_t sv_h, const int* __restrict__ kept_idx, const int* __restrict__ new_lens, const int* __restrict__ cu,
    const int* __restrict__ bh_lens0, const int* __restrict__ page_table, const int* __restrict__ bmap,
    uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, uint8_t* __restrict__ ksc, uint8_t* __restrict__ vsc, int H,
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
    mx_row_store<T, D>(key + (size_t)n * sk_n + h * sk_h, kc + prow * (D / 2), ksc + prow * (D / 32), dl);
    mx_row_store<T, D>(value + (size_t)n * sv_n + h * sv_h, vc + prow * (D / 2), vsc + prow * (D / 32), dl);
  }
}

// ---- compaction IN PLACE (last chunk of a chunked prefill on an MXFP4 cache) ----------------------------------------------
// Sibling of compact_inplace_kernel (store_kv.hip) and compact_inplace_fp8_kernel: the kept rows of every (b,h) move down
// to slots dst_base.. in token order.  The bits move as they are - D/2 code bytes and D/32 scale bytes, for K and for V,
// nothing is re-quantised - so the result is what compact_store_mxfp4_kernel writes from the packed 16-bit rows, byte for
// byte.  The no-overlap argument is that kernel's: with an ascending kept list slot j receives the row of token t_j >= j,
// tile i writes slots below dst_base + TILE (i + 1) and every source of a later tile lies at or above
// src_base + TILE (i + 1); inside a tile a barrier separates all loads from all stores, and the next tile's loads are
// issued before this tile's stores.
// A row is D/32 lanes; lane dl carries 16 B of codes = 32 elements = scale block dl, and that block's scale byte.
template <int D>
__global__ __launch_bounds__(256) void compact_inplace_mxfp4_kernel(
    const int* __restrict__ kept_idx, const int* __restrict__ new_lens, const int* __restrict__ dst_base,
    const int* __restrict__ src_base, const int* __restrict__ page_table, const int* __restrict__ bmap,
    uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, uint8_t* __restrict__ ksc, uint8_t* __restrict__ vsc, int H,
    int max_seqlen, int PS, int NLP) {
  constexpr int RB = D / 2;           // code bytes per row
  constexpr int LPR = D / 32;         // lanes per row = scale bytes per row
  constexpr int RPP = 256 / LPR;      // rows per pass of the workgroup
  constexpr int TILE = 128;           // rows per tile, as the siblings
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
    uint8_t ks[PASSES], vs[PASSES];
  };
  Rows buf[2];
  auto load_tile = [&](int t0, Rows& x) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int j = t0 + p * RPP + rl;
      if (j < cnt) {
        const size_t a = row_of(s0 + max(0, min(list[j], tok_max)));  // clamped: see compact_store_kernel
        x.k[p] = *reinterpret_cast<const uint4*>(kc + a * RB + dl * 16);
        x.v[p] = *reinterpret_cast<const uint4*>(vc + a * RB + dl * 16);
        x.ks[p] = ksc[a * LPR + dl];
        x.vs[p] = vsc[a * LPR + dl];
      }
    }
  };
  auto store_tile = [&](int t0, const Rows& x) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int j = t0 + p * RPP + rl;
      if (j < cnt) {
        const size_t a = row_of(d0 + j);
        *reinterpret_cast<uint4*>(kc + a * RB + dl * 16) = x.k[p];
        *reinterpret_cast<uint4*>(vc + a * RB + dl * 16) = x.v[p];
        ksc[a * LPR + dl] = x.ks[p];
        vsc[a * LPR + dl] = x.vs[p];
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
__device__ __forceinline__ void mx_vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Ring reads are inline asm with their own lgkmcnt wait (kv_fp8.hip): hipcc would otherwise drain vmcnt(0) in front of
// every LDS read while an LDS-DMA is pending.  One call reads what the logits of a unit need plus the V scales:
// K codes of the lane's two rows, their scale bytes, and the scale bytes of the eight rows of the lane's quarter.
__device__ __forceinline__ void mx_read_unit(uint32_t k0, uint32_t k1, uint32_t s0, uint32_t s1, uint32_t v0, uint32_t v1,
                                             u32x4_t& kd0, u32x4_t& kd1, uint32_t& ks0, uint32_t& ks1, u32x4_t& vs0,
                                             u32x4_t& vs1) {  // D = 128: 16 B of codes per row, 4 scale bytes per row
  asm volatile(
      "ds_read_b128 %0, %6\n\tds_read_b128 %1, %7\n\tds_read_u8 %2, %8\n\tds_read_u8 %3, %9\n\t"
      "ds_read_b128 %4, %10\n\tds_read_b128 %5, %11\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(kd0), "=&v"(kd1), "=&v"(ks0), "=&v"(ks1), "=&v"(vs0), "=&v"(vs1)
      : "v"(k0), "v"(k1), "v"(s0), "v"(s1), "v"(v0), "v"(v1)
      : "memory");
}
__device__ __forceinline__ void mx_read_unit(uint32_t k0, uint32_t k1, uint32_t s0, uint32_t s1, uint32_t v0, uint32_t v1,
                                             u32x2_t& kd0, u32x2_t& kd1, uint32_t& ks0, uint32_t& ks1, u32x2_t& vs0,
                                             u32x2_t& vs1) {  // D = 64: 8 B of codes per row, 2 scale bytes per row
  asm volatile(
      "ds_read_b64 %0, %6\n\tds_read_b64 %1, %7\n\tds_read_u8 %2, %8\n\tds_read_u8 %3, %9\n\t"
      "ds_read_b64 %4, %10\n\tds_read_b64 %5, %11\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(kd0), "=&v"(kd1), "=&v"(ks0), "=&v"(ks1), "=&v"(vs0), "=&v"(vs1)
      : "v"(k0), "v"(k1), "v"(s0), "v"(s1), "v"(v0), "v"(v1)
      : "memory");
}
// transposing read: inside a block of 16 lanes, lane t receives byte (t & 7) of the 8 bytes addressed by each of the
// lanes 2e + (t >> 3), e = 0..7
__device__ __forceinline__ void mx_read_tr8(const uint32_t (&a)[4], i32x2_t (&r)[4]) {
  asm volatile(
      "ds_read_b64_tr_b8 %0, %4\n\tds_read_b64_tr_b8 %1, %5\n\tds_read_b64_tr_b8 %2, %6\n\t"
      "ds_read_b64_tr_b8 %3, %7\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3])
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3])
      : "memory");
}
__device__ __forceinline__ void mx_read_tr8(const uint32_t (&a)[2], i32x2_t (&r)[2]) {
  asm volatile("ds_read_b64_tr_b8 %0, %2\n\tds_read_b64_tr_b8 %1, %3\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(r[0]), "=&v"(r[1])
               : "v"(a[0]), "v"(a[1])
               : "memory");
}

// byte SEL of w = two e2m1 codes -> one packed pair in the MFMA input type, times 2^(exponent field of sc - 127)
template <typename T, int SEL>
__device__ __forceinline__ uint32_t fp4x2_to16(uint32_t w, float sc) {
  if constexpr (T::code == CVLLM_BF16)
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, SEL));
  else
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, SEL));
}
template <typename T>
__device__ __forceinline__ s16x8 fp4x8_to16(uint32_t w, float sc) {  // the 8 codes of one word, one scale
  const u32x4_t r = {fp4x2_to16<T, 0>(w, sc), fp4x2_to16<T, 1>(w, sc), fp4x2_to16<T, 2>(w, sc), fp4x2_to16<T, 3>(w, sc)};
  return __builtin_bit_cast(s16x8, r);
}

template <typename T>
__device__ __forceinline__ f32x4 mx_mfma(s16x8 a, s16x8 b, f32x4 c) {
  if constexpr (T::code == CVLLM_BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

constexpr int MX_NW = 4;      // waves per workgroup
constexpr int MX_UR = 32;     // rows per unit
constexpr int MX_PGREGS = 8;  // page ids windowed through registers: 8 x 64 pages

// chunk c of row r of a unit lives at chunk c ^ mx_swz(r).  With r = b4 b3 b2 b1 b0: a pass of the K reads sees 16 rows
// with b4 fixed, a pass of the transposing V reads sees the rows with b3 fixed; rows that share a 256 B bank window differ
// in (b2, b3, b4) at D = 128 (64 B rows) and in (b3, b4) at D = 64 (32 B rows), so swz must be one-to-one in those bits
// with either b4 or b3 held.
template <int D>
__device__ __forceinline__ constexpr int mx_swz(int r) {
  return D == 128 ? (((r >> 2) & 1) | ((((r >> 3) ^ (r >> 4)) & 1) << 1)) : (((r >> 3) ^ (r >> 4)) & 1);
}

template <typename T, int D, int R>
__global__ __launch_bounds__(MX_NW * 64) void decode_mxfp4_kernel(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
    const uint8_t* __restrict__ ksc, const uint8_t* __restrict__ vsc, const int* __restrict__ seq_lens,
    const int* __restrict__ page_table, const int* __restrict__ bmap, uint16_t* __restrict__ out,
    float* __restrict__ part_o, float* __restrict__ part_lse, int HKV, int G, int PS, int NLP, int S, float scale) {
  constexpr int NW = MX_NW, UR = MX_UR;
  constexpr int RB = D / 2;               // code bytes per row
  constexpr int NSB = D / 32;             // scale bytes per row = 16 B chunks per row = 32-dim blocks of the output
  constexpr int KVB = UR * RB;            // code bytes of K (and of V) per unit
  constexpr int NLK = KVB / 1024;         // DMA instructions per K (and per V) of a unit
  constexpr int NSW = UR * NSB / 4;       // dwords of K (and of V) scales per unit
  constexpr int UNIT_BYTES = 2 * KVB + 256;  // K codes | V codes | K scales (at +0) | V scales (at +128)
  constexpr int P = R - 1;                // units in flight ahead of the one being reduced
  constexpr int NDMA = 2 * NLK + 1;
  constexpr int NT_AUX = 2;               // non-temporal: the cache is read once per step
  constexpr float VF = (T::code == CVLLM_F16) ? 512.f : 1.f;  // P is carried times VF (f16 subnormals)
  typedef typename std::conditional<D == 128, u32x4_t, u32x2_t>::type kvec_t;  // D/8 bytes
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
  const int L = seq_lens[bh];
  // rows are dealt to the S splits in whole units, as decode_fp8_kernel does
  const int U = (L + UR - 1) / UR;
  const int start = (int)(((long long)s * U) / S) * UR;
  const int end = min((int)(((long long)(s + 1) * U) / S) * UR, L);
  float* po = part_o + ((size_t)(b * S + s) * HQ + h * G) * D;
  float* pl = part_lse + (size_t)(b * S + s) * HQ + h * G;

  if (start >= end) {  // empty split (covers L == 0): zeros / a split that weighs nothing
    if (S == 1) {
      for (int i = tid; i < G * D; i += NW * 64) out[((size_t)b * HQ + h * G) * D + i] = 0;
    } else if (tid < G) {
      pl[tid] = -INFINITY;
    }
    return;
  }

  // Q as the B operand: lane (head j, quarter g) holds, for MFMA m, the 8 dims that K's lane (row, g) holds for it:
  // dims g D/4 + 8 m .. + 7
  s16x8 qb[NSB];
#pragma unroll
  for (int m = 0; m < NSB; ++m) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);  // heads G..15: zero columns
    if (j < G) v = *reinterpret_cast<const uint4*>(q + ((size_t)b * HQ + h * G + j) * D + g * (D / 4) + 8 * m);
    qb[m] = __builtin_bit_cast(s16x8, v);
  }

  const int* pt = page_table + ((size_t)bt * HKV + h) * NLP;
  const int lp0 = start / PS;
  int pg_win = 0;  // first page of the register window, relative to lp0
  int pgreg[MX_PGREGS];
#pragma unroll
  for (int jj = 0; jj < MX_PGREGS; ++jj) {
    const int i = lp0 + lane + 64 * jj;
    pgreg[jj] = i < NLP ? pt[i] : 0;
  }
  // retire every ordinary load before the first LDS-DMA and hide the registers' origin (decode_fp8_kernel)
#pragma unroll
  for (int jj = 0; jj < MX_PGREGS; ++jj) asm volatile("" : "+v"(pgreg[jj]));
#pragma unroll
  for (int m = 0; m < NSB; ++m) asm volatile("" : "+v"(qb[m]));

  // ---- per-lane constants of the LDS image ----------------------------------------------------------------------------
  int soff[NLK];  // global byte offset (inside the unit's contiguous run) this lane fetches with DMA instruction i
#pragma unroll
  for (int i = 0; i < NLK; ++i) {
    const int n = i * 64 + lane;  // 16 B slot the lane's data lands in
    const int r = n / NSB, p = n % NSB;
    soff[i] = r * RB + ((p ^ mx_swz<D>(r)) * 16);
  }
  // scale DMA: lane l < 32 fetches dword l % NSW of the unit's K scales, lane 32 + l that of its V scales (at D = 64
  // lanes 16-31 repeat lanes 0-15; their copies land in the unused half of the 128 B)
  const uint8_t* scp = (lane < 32 ? ksc : vsc) + 4 * ((lane & 31) % NSW);
  // K: lane (row j of block rb, quarter g) reads bytes g D/8 .. of the row; its elements lie in scale block kblk
  const int kchunk = D == 128 ? g : g >> 1, ksub = D == 128 ? 0 : 8 * (g & 1), kblk = kchunk;
  uint32_t kaddr[2], ksaddr[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int r = 16 * rb + j;
    kaddr[rb] = r * RB + ((kchunk ^ mx_swz<D>(r)) * 16) + ksub;
    ksaddr[rb] = 2 * KVB + r * NSB + kblk;
  }
  // V: source lane t = j of quarter g addresses row 16 (t >> 3) + 4 g + ((t >> 1) & 3), bytes 8 (t & 1) of a 16 B chunk
  const int vrow = 4 * g + ((j >> 1) & 3) + 16 * (j >> 3);
  const uint32_t vbase = KVB + vrow * RB + 8 * (j & 1);
  const uint32_t vsw = mx_swz<D>(vrow) * 16;
  const uint32_t vsaddr = 2 * KVB + 128 + 4 * g * NSB;  // V scale bytes of rows 4g..4g+3; + 16 NSB: rows 16+4g..

  const int nunits = (end - start + UR - 1) / UR;
  const int njw = nunits > wave ? (nunits - wave + NW - 1) / NW : 0;  // units owned by this wave
  char* ring = smem + wave * (R * UNIT_BYTES);
  const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)ring;

  auto page_of = [&](int lpi_rel) {
    const int lpi = lpi_rel - pg_win;
    int pg = __builtin_amdgcn_readlane(pgreg[0], lpi & 63);
#pragma unroll
    for (int jj = 1; jj < MX_PGREGS; ++jj)
      if ((lpi >> 6) == jj) pg = __builtin_amdgcn_readlane(pgreg[jj], lpi & 63);
    return pg;
  };

  auto issue = [&](int jw) {  // wave-local unit jw -> ring slot jw % R
    const int row0 = start + (wave + jw * NW) * UR;  // multiple of 32, PS % 32 == 0: the unit lies inside one page
    const int lpi_rel = row0 / PS - lp0;
    if (lpi_rel - pg_win >= 64 * MX_PGREGS) {  // rare: a split longer than 512 pages; the window only moves forward
      pg_win = lpi_rel;
#pragma unroll
      for (int jj = 0; jj < MX_PGREGS; ++jj) {
        const int i = lp0 + pg_win + lane + 64 * jj;
        pgreg[jj] = i < NLP ? pt[i] : 0;
      }
#pragma unroll
      for (int jj = 0; jj < MX_PGREGS; ++jj) asm volatile("" : "+v"(pgreg[jj]));
    }
    const size_t prow = (size_t)page_of(lpi_rel) * PS + row0 % PS;
    const uint8_t* kp = kc + prow * RB;
    const uint8_t* vp = vc + prow * RB;
    char* slot = ring + (jw % R) * UNIT_BYTES;
#pragma unroll
    for (int i = 0; i < NLK; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kp + soff[i]),
                                       (__attribute__((address_space(3))) void*)(slot + i * 1024), 16, 0, NT_AUX);
#pragma unroll
    for (int i = 0; i < NLK; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vp + soff[i]),
                                       (__attribute__((address_space(3))) void*)(slot + KVB + i * 1024), 16, 0, NT_AUX);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(scp + prow * NSB),
                                     (__attribute__((address_space(3))) void*)(slot + 2 * KVB), 4, 0, NT_AUX);
  };

  // online-softmax state of head j (m is the same in the four quarters, l is the quarter's partial sum) and
  // acc[c][par][r] = O[head j][32 c + 2 (4 g + r) + par]
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 acc[NSB][2];
#pragma unroll
  for (int c = 0; c < NSB; ++c) acc[c][0] = acc[c][1] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int jw = 0; jw < P; ++jw)
    if (jw < njw) issue(jw);

  for (int jw = 0; jw < njw; ++jw) {
    if (jw + P < njw) {
      issue(jw + P);
      mx_vm_wait<NDMA * P>();
    } else {
      mx_vm_wait<0>();  // tail: drain
    }
    const uint32_t sl = ring_lds + (jw % R) * UNIT_BYTES;
    const int row0 = start + (wave + jw * NW) * UR;

    // ---- logits of 2 x 16 rows ----------------------------------------------------------------------------------------
    kvec_t kd[2], vs[2];
    uint32_t ksb[2];
    mx_read_unit(sl + kaddr[0], sl + kaddr[1], sl + ksaddr[0], sl + ksaddr[1], sl + vsaddr, sl + vsaddr + 16 * NSB, kd[0],
                 kd[1], ksb[0], ksb[1], vs[0], vs[1]);
    f32x4 sacc[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const float ksf = __uint_as_float(ksb[rb] << 23);  // 2^E of the lane's K block (a stale 255: NaN, selected away)
      sacc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int mm = 0; mm < NSB; ++mm) sacc[rb] = mx_mfma<T>(fp4x8_to16<T>(kd[rb][mm], ksf), qb[mm], sacc[rb]);
    }
    // lane (head j, quarter g) now holds the logits of rows row0 + 16 rb + 4 g + r
    float sv[8];
    bool ok[8];
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int rb = e >> 2, r = e & 3;
      ok[e] = row0 + 16 * rb + 4 * g + r < end;
      sv[e] = ok[e] ? sacc[rb][r] * scale : -INFINITY;
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
      pv[e] = ok[e] ? p * VF : 0.f;
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
      for (int c = 0; c < NSB; ++c) {
        acc[c][0] *= alpha;
        acc[c][1] *= alpha;
      }
    }
    // the scale bytes of contraction slot e, one word per slot (byte c = block c); rows past `end` (only in the split's
    // last unit) hold stale codes and scales: zero both (a zero scale word and zero codes convert to zeros)
    uint32_t vsc_w[8];
    uint32_t vm0 = 0xffffffffu, vm1 = 0xffffffffu;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if constexpr (D == 128) vsc_w[e] = vs[e >> 2][e & 3];
      else vsc_w[e] = (vs[e >> 2][(e & 3) >> 1] >> (16 * (e & 1))) & 0xffffu;
    }
    if (row0 + UR > end) {
      vm0 = (ok[0] ? 0xffu : 0u) | (ok[1] ? 0xff00u : 0u) | (ok[2] ? 0xff0000u : 0u) | (ok[3] ? 0xff000000u : 0u);
      vm1 = (ok[4] ? 0xffu : 0u) | (ok[5] ? 0xff00u : 0u) | (ok[6] ? 0xff0000u : 0u) | (ok[7] ? 0xff000000u : 0u);
#pragma unroll
      for (int e = 0; e < 8; ++e) vsc_w[e] = ok[e] ? vsc_w[e] : 0u;
    }
    // ---- O^T += V^T P^T -------------------------------------------------------------------------------------------------
    uint32_t va[NSB];
    i32x2_t vt[NSB];
#pragma unroll
    for (int c = 0; c < NSB; ++c) va[c] = sl + vbase + ((c * 16) ^ vsw);
    mx_read_tr8(va, vt);  // vt[c] byte e = (V[slot e][32 c + 2 j], V[slot e][32 c + 2 j + 1])
#pragma unroll
    for (int c = 0; c < NSB; ++c) {
      const uint32_t w0 = (uint32_t)vt[c][0] & vm0, w1 = (uint32_t)vt[c][1] & vm1;
      uint32_t pr[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        // exponent field <- byte c of the slot's scale word
        constexpr int SH = 23 - 8 * 3;  // byte 3 sits one bit above the exponent field
        const uint32_t sb = (c < 3 ? vsc_w[e] << ((23 - 8 * c) & 31) : vsc_w[e] >> -SH) & 0x7f800000u;
        const float sf = __uint_as_float(sb);
        const uint32_t w = e < 4 ? w0 : w1;
        pr[e] = (e & 3) == 0 ? fp4x2_to16<T, 0>(w, sf) : (e & 3) == 1 ? fp4x2_to16<T, 1>(w, sf)
                : (e & 3) == 2 ? fp4x2_to16<T, 2>(w, sf) : fp4x2_to16<T, 3>(w, sf);
      }
      u32x4_t ae, ao;  // low halves: the even dim of every slot; high halves: the odd dim
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ae[k] = (pr[2 * k] & 0xffffu) | (pr[2 * k + 1] << 16);
        ao[k] = (pr[2 * k] >> 16) | (pr[2 * k + 1] & 0xffff0000u);
      }
      const s16x8 sae = __builtin_bit_cast(s16x8, ae), sao = __builtin_bit_cast(s16x8, ao);
      acc[c][0] = mx_mfma<T>(sae, pbh, acc[c][0]);
      acc[c][1] = mx_mfma<T>(sao, pbh, acc[c][1]);
      acc[c][0] = mx_mfma<T>(sae, pbl, acc[c][0]);
      acc[c][1] = mx_mfma<T>(sao, pbl, acc[c][1]);
    }
  }

  // ---- merge of the NW waves' states -----------------------------------------------------------------------------------
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  constexpr int ST_ML = 8 * D * 4;  // (m, l) pairs behind the fp32 numerators of up to 8 heads
  static_assert(ST_ML + 64 <= R * UNIT_BYTES, "staging area must fit the wave's ring");
  if (j < G) {  // all of this wave's DMA has landed and been read
#pragma unroll
    for (int c = 0; c < NSB; ++c) {  // dims 32 c + 8 g .. + 7 in natural order: even / odd interleaved
      float* dst = reinterpret_cast<float*>(ring) + j * D + 32 * c + 8 * g;
      *reinterpret_cast<float4*>(dst) = make_float4(acc[c][0][0], acc[c][1][0], acc[c][0][1], acc[c][1][1]);
      *reinterpret_cast<float4*>(dst + 4) = make_float4(acc[c][0][2], acc[c][1][2], acc[c][0][3], acc[c][1][3]);
    }
    if (g == 0) *reinterpret_cast<float2*>(ring + ST_ML + j * 8) = make_float2(m_run, l_run);
  }
  __syncthreads();
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
    } else {  // normalised fp32 partial + natural-log LSE: what decode_stage2_kernel reads
      po[hd * D + d] = o;
      if (d == 0) pl[hd] = M + __logf(den);
    }
  }
}

template <typename T, int D>
static int launch_decode_mxfp4(const void* q, const void* kc, const void* vc, const uint8_t* ksc, const uint8_t* vsc,
                               void* out, const int* seq_lens, const int* page_table, const int* bmap, char* ws, int B,
                               int HQ, int HKV, int PS, int NLP, float scale, int S, hipStream_t st) {
  constexpr int R = D == 128 ? 8 : 12;
  constexpr size_t smem = (size_t)MX_NW * R * (2 * MX_UR * (D / 2) + 256);
  static_assert(smem <= 160 * 1024, "LDS budget");
  float* part_o = S > 1 ? reinterpret_cast<float*>(ws + DEC_WS_HEADER) : nullptr;
  float* part_lse = S > 1 ? part_o + (size_t)B * S * HQ * D : nullptr;
  auto kern = decode_mxfp4_kernel<T, D, R>;
  set_dyn_lds_once(kern, (int)smem);
  hipLaunchKernelGGL(kern, dim3(B * HKV * S), dim3(MX_NW * 64), smem, st, (const uint16_t*)q, (const uint8_t*)kc,
                     (const uint8_t*)vc, ksc, vsc, seq_lens, page_table, bmap, (uint16_t*)out, part_o, part_lse, HKV,
                     HQ / HKV, PS, NLP, S, scale);
  if (S > 1) return launch_decode_stage2(part_o, part_lse, out, B, HQ, D, S, T::code, st);
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

extern "C" int cvllm_store_decode_kv_mxfp4(const void* key, const void* value, int64_t sk_b, int64_t sk_h, int64_t sv_b,
                                           int64_t sv_h, const int32_t* batch_mapping, int32_t* bh_lens,
                                           const int32_t* page_table, void* k_cache, void* v_cache, int B, int HKV,
                                           int D, int page_size, int n_logical_pages_max, int reserved_batch, int dtype,
                                           cvllm_stream_t stream, uint8_t* k_scale, uint8_t* v_scale) {
  if (!key || !value || !batch_mapping || !bh_lens || !page_table || !k_cache || !v_cache || !k_scale || !v_scale)
    return CVLLM_ERR_ARG;
  if (B <= 0 || HKV <= 0 || page_size <= 0 || n_logical_pages_max <= 0) return CVLLM_ERR_ARG;
  if ((sk_b % 8) || (sk_h % 8) || (sv_b % 8) || (sv_h % 8)) return CVLLM_ERR_SHAPE;  // 16 B source loads
  hipStream_t st = (hipStream_t)stream;
  const int BH = B * HKV;
  DISPATCH_TD(dtype, D, {
    const int rpb = 256 / (DD / 16);
    hipLaunchKernelGGL((decode_store_mxfp4_kernel<TT, DD>), dim3((BH + rpb - 1) / rpb), dim3(256), 0, st,
                       (const uint16_t*)key, (const uint16_t*)value, sk_b, sk_h, sv_b, sv_h, batch_mapping, bh_lens,
                       page_table, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale, v_scale, BH, HKV, page_size,
                       n_logical_pages_max, reserved_batch);
  });
  return check_launch();
}

extern "C" int cvllm_store_all_kv_mxfp4(const void* new_keys, const void* new_values, int64_t sk_n, int64_t sk_h,
                                        int64_t sv_n, int64_t sv_h, const int32_t* cu_seqlens_k,
                                        const int32_t* batch_mapping, int32_t* bh_lens, const int32_t* page_table,
                                        void* k_cache, void* v_cache, int B, int total_tokens, int HKV, int D,
                                        int page_size, int n_logical_pages_max, int dtype, cvllm_stream_t stream,
                                        uint8_t* k_scale, uint8_t* v_scale) {
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
      hipLaunchKernelGGL((store_all_mxfp4_kernel<TT, DD>), dim3((int)blocks), dim3(256), 0, st,
                         (const uint16_t*)new_keys, (const uint16_t*)new_values, sk_n, sk_h, sv_n, sv_h, cu_seqlens_k,
                         batch_mapping, bh_lens, page_table, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale, v_scale, B,
                         total_tokens, HKV, page_size, n_logical_pages_max);
    });
  } else if ((dtype != CVLLM_F16 && dtype != CVLLM_BF16) || (D != 64 && D != 128)) {
    return CVLLM_ERR_SHAPE;
  }
  hipLaunchKernelGGL(add_seq_lens_mxfp4_kernel, dim3((B * HKV + 255) / 256), dim3(256), 0, st, cu_seqlens_k, bh_lens, B,
                     HKV);
  return check_launch();
}

extern "C" int cvllm_compact_store_mxfp4(const void* new_keys, const void* new_vals, int64_t sk_n, int64_t sk_h,
                                         int64_t sv_n, int64_t sv_h, const int32_t* kept_idx, const int32_t* new_lens,
                                         const int32_t* cu_seqlens_k, const int32_t* bh_lens0,
                                         const int32_t* page_table, const int32_t* batch_mapping, void* k_cache,
                                         void* v_cache, int B, int H, int D, int max_seqlen, int page_size,
                                         int n_logical_pages_max, int dtype, cvllm_stream_t stream, uint8_t* k_scale,
                                         uint8_t* v_scale) {
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
    hipLaunchKernelGGL((compact_store_mxfp4_kernel<TT, DD>), dim3(B * H * tiles), dim3(256), 0, st,
                       (const uint16_t*)new_keys, (const uint16_t*)new_vals, sk_n, sk_h, sv_n, sv_h, kept_idx, new_lens,
                       cu_seqlens_k, bh_lens0, page_table, batch_mapping, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale,
                       v_scale, H, max_seqlen, page_size, n_logical_pages_max, tiles);
  });
  return check_launch();
}

extern "C" int cvllm_compact_cache_inplace_mxfp4(const int32_t* kept_idx, const int32_t* new_lens,
                                                 const int32_t* dst_base, const int32_t* src_base,
                                                 const int32_t* page_table, const int32_t* batch_mapping,
                                                 void* k_cache, void* v_cache, int B, int H, int D, int max_seqlen,
                                                 int page_size, int n_logical_pages_max, cvllm_stream_t stream,
                                                 uint8_t* k_scale, uint8_t* v_scale) {
  if (!kept_idx || !new_lens || !dst_base || !src_base || !page_table || !batch_mapping || !k_cache || !v_cache ||
      !k_scale || !v_scale)
    return CVLLM_ERR_ARG;
  if (B <= 0 || H <= 0 || max_seqlen <= 0 || page_size <= 0 || n_logical_pages_max <= 0) return CVLLM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
#define CI_CALL(D_)                                                                                                   \
  hipLaunchKernelGGL((compact_inplace_mxfp4_kernel<D_>), dim3(B* H), dim3(256), 0, st, kept_idx, new_lens, dst_base,  \
                     src_base, page_table, batch_mapping, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale, v_scale, H,  \
                     max_seqlen, page_size, n_logical_pages_max)
  if (D == 64) CI_CALL(64);
  else if (D == 128) CI_CALL(128);
  else return CVLLM_ERR_SHAPE;
#undef CI_CALL
  return check_launch();
}

extern "C" int cvllm_decode_attn_mxfp4(const void* q, const void* k_cache, const void* v_cache, const uint8_t* k_scale,
                                       const uint8_t* v_scale, void* out, const int32_t* seq_lens_bh,
                                       const int32_t* page_table, const int32_t* batch_mapping, void* workspace,
                                       size_t workspace_bytes, int B, int HQ, int HKV, int D, int page_size,
                                       int n_logical_pages_max, float sm_scale, int n_splits, int dtype,
                                       cvllm_stream_t stream) {
  if (!q || !k_cache || !v_cache || !k_scale || !v_scale || !out || !seq_lens_bh || !page_table || !batch_mapping)
    return CVLLM_ERR_ARG;
  if (B <= 0 || HQ <= 0 || HKV <= 0 || n_splits <= 0 || n_logical_pages_max <= 0) return CVLLM_ERR_ARG;
  if (HQ % HKV != 0 || n_splits > 256) return CVLLM_ERR_SHAPE;
  const int G = HQ / HKV;
  if (G != 1 && G != 2 && G != 4 && G != 8) return CVLLM_ERR_SHAPE;
  if (page_size <= 0 || page_size % MX_UR != 0) return CVLLM_ERR_SHAPE;  // a unit of 32 rows must not straddle a page
  if (D != 64 && D != 128) return CVLLM_ERR_SHAPE;
  if (n_splits > 1 && (!workspace || workspace_bytes < cvllm_decode_workspace_bytes(B, HQ, D, n_splits)))
    return CVLLM_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_TD(dtype, D, {
    return (launch_decode_mxfp4<TT, DD>(q, k_cache, v_cache, k_scale, v_scale, out, seq_lens_bh, page_table,
                                        batch_mapping, (char*)workspace, B, HQ, HKV, page_size, n_logical_pages_max,
                                        sm_scale, n_splits, st));
  });
  return CVLLM_ERR_SHAPE;
}
