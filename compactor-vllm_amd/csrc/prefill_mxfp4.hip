// Causal varlen prefill attention over [MXFP4 paged per-head prefix || 16-bit appended block], GQA, gfx950 MFMA.
//
// What chunked prefill and prefix reuse need on an MXFP4 cache (DESIGN.md sections 2 and 3.2.2): the cached prefix is
// e2m1 codes, two per byte, + one e8m0 scale byte per 32 elements (kv_mxfp4.hip); the appended block is the model's
// 16-bit k / v as in prefill_attn.hip.
//
// Structure: the compiler-scheduled 8-wave kernel of prefill_attn.hip - a workgroup = 256 query rows = (256/G tokens) x G
// heads of one kv-head, 64-key tiles (cached tiles first, then appended tiles up to the diagonal), S^T = K Q^T and
// O^T += V^T P^T with v_mfma_f32_32x32x16, V^T by ds_read_b64_tr_b16, K double- and V triple-buffered padded 16-bit LDS
// images, one barrier per tile, the in-wave software pipeline, exp2-domain online softmax with the deferred rescale.  The
// tile loop is that kernel's, line for line: it carries no scale and no conversion.
//
// What is new is the STAGING of a cached tile.  A 64-row tile is 64 x D/2 code bytes and 64 x D/32 scale bytes per
// operand - at D = 128 4 KiB + 256 B, a quarter of a 16-bit tile's global bytes - and a thread's share of it is 16
// elements: HALF a scale block.
//   * D = 128: thread (row = tid / 8, chunk = tid % 8) loads 8 B of K codes and 8 B of V codes of ONE row (elements
//     16 chunk .. + 15) and the scale byte of block chunk / 2 of each.
//   * D = 64: a row has only four such chunks per operand, so the eight threads of a row split by operand: chunks 0-3
//     stage K, chunks 4-7 stage V (8 B of codes and one scale byte each).  All 512 threads work, each half as much.
//   * conversion: one v_cvt_scalef32_pk_{bf16,f16}_fp4 per code byte, eight per operand, with the fp32 whose exponent
//     field is the scale byte as the scale operand (decode_mxfp4_kernel's construction): the block's 2^E folds in exactly,
//     there is no multiply and no separate rounding.  The sixteen results go out as 2 x 16 B into the SAME padded images.
//   * appended tile: the 16-bit kernel's mapping (rows r, r + 32; 16 B chunk), copied through.
// Both kinds go through the same registers and the same software pipeline (global loads of tile t + 2 at the top of
// iteration t, its LDS writes at the end); which kind a staged tile is, is workgroup-uniform (t < ntc).
//
// Read-back rule: fp32(code) * 2^E - exact in bf16, exact in f16 inside f16's normal range and unspecified outside it
// (DESIGN.md section 2); no extra rounding, unlike the FP8 prefix's rne_T(code * scale).
//
// Paging and ragged ends are the 16-bit kernel's: the scalar incremental page walk when PS % 64 == 0, a per-row lookup
// otherwise; rows past the end of a tile are CLAMPED to the tile's last valid row (their logits are masked to -inf), so a
// cache row beyond a head's length - any code byte, any scale byte, the NaN scale 0xFF included - is never read.
#include "common.h"

namespace cvllm {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// ---- the 8-wave kernel's helpers and constants (prefill_attn.hip, which is not to be touched; same definitions) ---------
template <typename T>
__device__ __forceinline__ f32x16 mfma32(s16x8 a, s16x8 b, f32x16 c);
template <>
__device__ __forceinline__ f32x16 mfma32<F16>(s16x8 a, s16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x16 mfma32<BF16>(s16x8 a, s16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
                                                 0);
}

constexpr int MXP_THR = 8;       // rescale threshold, exp2 domain (PF_THR)
constexpr int MXP_ROWS = 256;    // query rows per workgroup
constexpr int MXP_KT = 64;       // keys per tile
constexpr int MXP_THREADS = 512;
constexpr int MXP_KSTR = 272;    // K image row stride: 256 + 16 B pad -> conflict-free ds_read_b128
constexpr int MXP_VSTR = 320;    // V image row stride: 256 + 64 B pad -> conflict-free ds_read_b64_tr_b16
constexpr int MXP_KTILE = MXP_KT * MXP_KSTR;
constexpr int MXP_VTILE = MXP_KT * MXP_VSTR;
constexpr int MXP_OSTRIDE = 272;
constexpr int MXP_SMEM = 2 * MXP_KTILE + 3 * MXP_VTILE;  // 96,256 B
static_assert(MXP_SMEM >= 8 * 32 * MXP_OSTRIDE, "O staging image must fit");

// built with -fno-honor-nans (build.py), as prefill_attn.hip: one v_max3 per two MFMA results instead of a canonicalising
// v_max x,x in front of every operand
__device__ __forceinline__ float max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
__device__ __forceinline__ float tile_max(const f32x16& a, const f32x16& b) {
  float m0 = max3(a[0], a[1], a[2]), m1 = max3(b[0], b[1], b[2]);
#pragma unroll
  for (int i = 3; i < 15; i += 2) m0 = max3(m0, a[i], a[i + 1]), m1 = max3(m1, b[i], b[i + 1]);
  const float mx = max3(m0, m1, fmaxf(a[15], b[15]));
  const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
  return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- 16 e2m1 codes (8 bytes) of one row, all inside ONE scale block -> 16 values of the model dtype, 2 x 16 B into an
// LDS image.  Byte i holds element 2 i in its low nibble; the conversion returns (low nibble, high nibble) as the
// (low, high) halves of a dword, each times 2^(exponent field of sc - 127).
template <typename T, int SEL>
__device__ __forceinline__ uint32_t fp4x2_to16(uint32_t w, float sc) {
  if constexpr (T::code == CVLLM_BF16)
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, SEL));
  else
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, SEL));
}
template <typename T>
__device__ __forceinline__ void dequant16_to_lds(uint32_t c0, uint32_t c1, uint32_t scale_byte, char* dst) {
  const float sc = __uint_as_float(scale_byte << 23);  // 2^E
  *reinterpret_cast<uint4*>(dst) = make_uint4(fp4x2_to16<T, 0>(c0, sc), fp4x2_to16<T, 1>(c0, sc),
                                              fp4x2_to16<T, 2>(c0, sc), fp4x2_to16<T, 3>(c0, sc));
  *reinterpret_cast<uint4*>(dst + 16) = make_uint4(fp4x2_to16<T, 0>(c1, sc), fp4x2_to16<T, 1>(c1, sc),
                                                   fp4x2_to16<T, 2>(c1, sc), fp4x2_to16<T, 3>(c1, sc));
}

template <typename T, int D, int G>
__global__ __launch_bounds__(MXP_THREADS) void prefill_attn_mxfp4_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, int64_t sq_n,
    int64_t sk_n, int64_t sk_h, int64_t sv_n, int64_t sv_h, const uint8_t* __restrict__ kc,
    const uint8_t* __restrict__ vc, const uint8_t* __restrict__ ksc, const uint8_t* __restrict__ vsc,
    uint16_t* __restrict__ out, const int* __restrict__ seq_lens, const int* __restrict__ page_table,
    const int* __restrict__ bmap, const int* __restrict__ cu, int B, int HKV, int PS, int NLP, float scale_log2e) {
  constexpr int BM = MXP_ROWS / G;  // tokens per query tile
  constexpr int KS = D / 16;        // k-steps of the QK^T product
  constexpr int DB = D / 32;        // 32-wide blocks of the head dim
  constexpr int CH = D / 8;         // 16-byte chunks per 16-bit row
  constexpr int RB = D / 2;         // code bytes per cache row
  constexpr int NSB = D / 32;       // scale bytes per cache row
  constexpr int CH4 = D / 16;       // 8-byte (16-code) chunks per row of codes: 8 at D = 128, 4 at D = 64
  static_assert(D == 64 || D == 128, "head dim");

  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int bid = blockIdx.x;
  const int g = bid % HKV;
  const int b = (bid / HKV) % B;
  const int tile_rev = bid / (HKV * B);
  const int s0 = cu[b];
  const int La = cu[b + 1] - s0;
  const int nqt = (La + BM - 1) / BM;
  if (tile_rev >= nqt) return;
  const int qt = nqt - 1 - tile_rev;  // heaviest tiles first
  const int m0 = qt * BM;
  const int HQ = HKV * G;

  const int Lc = seq_lens[b * HKV + g];
  const int* pt = page_table + ((size_t)bmap[b] * HKV + g) * NLP;

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int row = wave * 32 + r;            // query row inside the tile
  const int head_local = row / BM;
  const int tok = m0 + row % BM;            // local token index of this lane's query
  const bool valid_q = tok < La;
  const int hq = g * G + head_local;

  // ---- Q fragments (B operand: lane holds Q[q = r][dims 16s + 8h .. +8]) ---------------------------------
  s16x8 qf[KS];
  {
    const uint16_t* qp = q + (size_t)(s0 + (valid_q ? tok : 0)) * sq_n + (size_t)hq * D + 8 * h;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      uint4 t = valid_q ? *reinterpret_cast<const uint4*>(qp + 16 * s) : make_uint4(0, 0, 0, 0);
      qf[s] = __builtin_bit_cast(s16x8, t);
    }
  }

  const int ntc = (Lc + MXP_KT - 1) / MXP_KT;                     // cached-prefix tiles (MXFP4)
  const int la_vis = min(m0 + BM, La);                            // appended keys visible to this query tile
  const int nta = (la_vis + MXP_KT - 1) / MXP_KT;                 // appended tiles (16 bit; the last ones are on the diagonal)
  const int ntiles = ntc + nta;

  // ---- staging ---------------------------------------------------------------------------------------------------------
  // appended (16-bit) tile: thread -> (rows srow, srow + 32; 16 B chunk sch), four registers kr0 kr1 vr0 vr1
  // cached (MXFP4) tile:    thread -> (row fr = tid / 8; fc = tid % 8), 8 B of codes = 16 elements = half a scale block:
  //   D = 128: chunk fc of K AND of V: kr0[0..1] = K codes, vr0[0..1] = V codes, ksr / vsr = scale byte of block fc / 2
  //   D = 64:  chunk fc % 4 of ONE operand (fc < 4: K, else V): kr0[0..1] = its codes, ksr = scale byte of block (fc % 4) / 2
  const int sch = tid & 15;
  const int srow = tid >> 4;  // 0..31
  const bool stage_active = sch < CH;
  u32x4 kr0, kr1, vr0, vr1;  // named scalars (arrays captured by the lambdas go to scratch)
  uint32_t ksr = 0u, vsr = 0u;
  // Beyond the two scale bytes the MXFP4 mapping keeps NO register live across the MFMA loop (the 16-bit kernel sits at
  // the 256-register limit already): its lane constants are recomputed from a laundered copy of tid where they are used (a
  // handful of VALU per tile) and the loads are uniform base + 32-bit lane offset.  A cached tile uses 2 (D = 64) or 4 of
  // the 16 staging dwords and says so (mx_kill, before its loads): carried through as live values the others make hipcc
  // land the appended tiles' loads in other registers and copy them over behind a vmcnt(0) at the top of the iteration.
  auto mx_kill = [&]() { asm volatile("" : "=v"(kr0), "=v"(kr1), "=v"(vr0), "=v"(vr1)); };
  auto mx_lane = [&](int& fr, int& fc) {
    int tl = tid;
    asm volatile("" : "+v"(tl));
    fr = tl >> 3;  // row of the tile, 0..63
    fc = tl & 7;
  };

  // Rows past the end of a tile are clamped to its last valid row, never skipped and never read from beyond the head's
  // length: their logits are masked to -inf (P = 0) and the clamped row is finite data, so 0 * V stays 0.
  const bool ps64 = (PS % MXP_KT) == 0;
  int ld_pi = 0, ld_po = 0;                 // page index / offset in page of the next cached tile to load
  int ld_pg = (ntc > 0) ? pt[0] : 0;        // its physical page
  const uint32_t skn = (uint32_t)sk_n, svn = (uint32_t)sv_n;  // row strides < 2^31 elements (checked on the host)
  auto gload = [&](int t) {
    if (t < ntc) {
      int fr, fc;
      mx_lane(fr, fc);
      size_t base;   // physical cache row (index of the codes' row AND of its scales): workgroup-uniform part
      uint32_t rl;   // ... and the lane's part
      if (ps64) {
        base = (size_t)ld_pg * PS + ld_po;
        rl = (uint32_t)min(fr, Lc - 1 - t * MXP_KT);  // last valid row of the tile, >= 0
        ld_po += MXP_KT;
        if (ld_po >= PS) {
          ld_po = 0;
          ld_pi += 1;
          ld_pg = pt[min(ld_pi, NLP - 1)];
        }
      } else {
        const int p = min(t * MXP_KT + fr, Lc - 1);
        base = (size_t)pt[p / PS] * PS + p % PS;
        rl = 0;
      }
      mx_kill();
      const uint32_t c4 = (uint32_t)fc % CH4;  // 16-code chunk of the row
      const uint32_t off = rl * RB + c4 * 8, soff = rl * NSB + c4 / 2;
      if constexpr (D == 128) {
        const uint2 kw = *reinterpret_cast<const uint2*>(kc + base * RB + off);
        const uint2 vw = *reinterpret_cast<const uint2*>(vc + base * RB + off);
        ksr = (ksc + base * NSB)[soff];
        vsr = (vsc + base * NSB)[soff];
        kr0[0] = kw.x, kr0[1] = kw.y, vr0[0] = vw.x, vr0[1] = vw.y;
      } else {
        const bool is_v = fc >= CH4;
        const uint2 cw = *reinterpret_cast<const uint2*>((is_v ? vc : kc) + base * RB + off);
        ksr = ((is_v ? vsc : ksc) + base * NSB)[soff];
        kr0[0] = cw.x, kr0[1] = cw.y;
      }
    } else if (stage_active) {
      const uint32_t n0 = (uint32_t)(s0 + min((t - ntc) * MXP_KT + srow, la_vis - 1));
      const uint32_t n1 = (uint32_t)(s0 + min((t - ntc) * MXP_KT + srow + 32, la_vis - 1));
      const uint16_t* kg = k + (size_t)g * sk_h + sch * 8;
      const uint16_t* vg = v + (size_t)g * sv_h + sch * 8;
      kr0 = *reinterpret_cast<const u32x4*>(kg + (uint64_t)n0 * skn);
      kr1 = *reinterpret_cast<const u32x4*>(kg + (uint64_t)n1 * skn);
      vr0 = *reinterpret_cast<const u32x4*>(vg + (uint64_t)n0 * svn);
      vr1 = *reinterpret_cast<const u32x4*>(vg + (uint64_t)n1 * svn);
    }
  };

  // ---- accumulators --------------------------------------------------------------------------------------------
  f32x16 oacc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;
  float m_run = -INFINITY;  // running max (exp2 domain), identical in lanes l and l^32
  float l_run = 0.f;        // running sum of this lane's half of the keys

  const int gi = lane >> 4;
  const int li = lane & 15;
  const int tq = li >> 2, tp = li & 3;

  char* const kbase = smem;
  char* const vbase = smem + 2 * MXP_KTILE;
  const uint32_t kst = srow * MXP_KSTR + sch * 16, vst = srow * MXP_VSTR + sch * 16;
  // tile t (the one the staging registers hold) -> K buffer kbuf, V buffer vbuf
  auto lstore = [&](int t, int kbuf, int vbuf) {
    if (t < ntc) {
      int fr, fc;
      mx_lane(fr, fc);
      if constexpr (D == 128) {
        dequant16_to_lds<T>(kr0[0], kr0[1], ksr, kbase + kbuf * MXP_KTILE + fr * MXP_KSTR + fc * 32);
        dequant16_to_lds<T>(vr0[0], vr0[1], vsr, vbase + vbuf * MXP_VTILE + fr * MXP_VSTR + fc * 32);
      } else {
        char* dst = fc >= CH4 ? vbase + vbuf * MXP_VTILE + fr * MXP_VSTR + (fc - CH4) * 32
                              : kbase + kbuf * MXP_KTILE + fr * MXP_KSTR + fc * 32;
        dequant16_to_lds<T>(kr0[0], kr0[1], ksr, dst);
      }
    } else if (stage_active) {
      char* kb = kbase + kbuf * MXP_KTILE + kst;
      char* vb = vbase + vbuf * MXP_VTILE + vst;
      *reinterpret_cast<u32x4*>(kb) = kr0;
      *reinterpret_cast<u32x4*>(kb + 32 * MXP_KSTR) = kr1;
      *reinterpret_cast<u32x4*>(vb) = vr0;
      *reinterpret_cast<u32x4*>(vb + 32 * MXP_VSTR) = vr1;
    }
  };
  const uint32_t k_lane = r * MXP_KSTR + h * 16;                                           // + 32 s (+ 32 rows)
  const uint32_t v_lane = (4 * (gi >> 1) + tq) * MXP_VSTR + (gi & 1) * 32 + tp * 8;       // + rows, + 64 db
  typedef __attribute__((address_space(3))) char lds_char;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_char*)smem;  // LDS byte address of the dynamic segment
  // tile base added to the lane constant ONCE and laundered: every read is that VGPR plus an immediate
  auto qk_tile = [&](int kbuf, f32x16& s0_, f32x16& s1_) {
    uint32_t ka = lds0 + kbuf * MXP_KTILE + k_lane;
    asm volatile("" : "+v"(ka));
    const lds_char* kb = (const lds_char*)(uintptr_t)ka;
#pragma unroll
    for (int i = 0; i < 16; ++i) s0_[i] = 0.f, s1_[i] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const s16x8 a0 = *reinterpret_cast<const __attribute__((address_space(3))) s16x8*>(kb + 32 * s);
      const s16x8 a1 = *reinterpret_cast<const __attribute__((address_space(3))) s16x8*>(kb + 32 * s + 32 * MXP_KSTR);
      s0_ = mfma32<T>(a0, qf[s], s0_);
      s1_ = mfma32<T>(a1, qf[s], s1_);
    }
  };

  // ---- main loop: prefill_attn_kernel's, one 64-key tile per iteration, software-pipelined by one tile -------------------
  // K(t+2) replaces K(t) (last read in iteration t-1), V(t+2) replaces V(t-1); global loads of tile t+2 at the top of
  // iteration t, its LDS writes - with the conversion, if it is a cached tile - at the end, behind ONE barrier per tile.
  // The switch from 4-bit to 16-bit staging happens between two tiles of this pipeline: gload(t) and lstore(t, ..) decide
  // by the same test on the same t, so the registers a tile was loaded into are read back the way they were filled.
  kr0 = kr1 = vr0 = vr1 = u32x4{0u, 0u, 0u, 0u};
  gload(0);
  lstore(0, 0, 0);
  if (ntiles > 1) gload(1);
  lds_barrier();
  f32x16 sc0, sc1;  // raw logits of the current tile (keys 0-31 / 32-63)
  qk_tile(0, sc0, sc1);
  float mx_raw = tile_max(sc0, sc1);
  if (ntiles > 1) lstore(1, 1, 1);
  lds_barrier();

  int vcur = 0;  // t % 3
  for (int t = 0; t < ntiles; ++t) {
    if (t + 2 < ntiles) gload(t + 2);

    const int vnext2 = vcur == 0 ? 2 : vcur - 1;  // (t + 2) % 3

    const bool cached = t < ntc;
    const int j0 = cached ? t * MXP_KT : (t - ntc) * MXP_KT;
    const int count = cached ? min(MXP_KT, Lc - j0) : min(MXP_KT, la_vis - j0);
    const bool need_mask = count < MXP_KT || (!cached && j0 + MXP_KT - 1 > m0);  // wave-uniform
    if (need_mask) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kk = (i & 3) + 8 * (i >> 2) + 4 * h;
        const bool vis0 = kk < count && (cached || (j0 + kk) <= tok);
        const bool vis1 = kk + 32 < count && (cached || (j0 + kk + 32) <= tok);
        sc0[i] = vis0 ? sc0[i] : -INFINITY;
        sc1[i] = vis1 ? sc1[i] : -INFINITY;
      }
    }
    if (need_mask) mx_raw = tile_max(sc0, sc1);
    const float mx = mx_raw * scale_log2e;
    // deferred rescale: the running max follows the row max only once it has grown by more than MXP_THR (exp2 domain)
    const bool grew = mx > m_run + (float)MXP_THR;
    const float m_new = grew ? mx : m_run;
    const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_safe);
    m_run = m_new;
    if (__any(grew)) {  // alpha == 1 for every lane otherwise
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[db][i] *= alpha;
    }

    // ---- S(t+1) = K(t+1) Q^T  (MFMA)   ||   P(t) = exp2(S(t) c - m) packed to the model dtype  (VALU) -----------
    // On the last tile this recomputes an old K tile; the result is never used.
    f32x16 sn0, sn1;
    qk_tile((t + 1) & 1, sn0, sn1);

    float psum = 0.f;
    s16x8 pf[4];
#pragma unroll
    for (int kb2 = 0; kb2 < 2; ++kb2) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        uint32_t w[4];
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {
          const float x0 = kb2 ? sc1[8 * s2 + 2 * jp] : sc0[8 * s2 + 2 * jp];
          const float x1 = kb2 ? sc1[8 * s2 + 2 * jp + 1] : sc0[8 * s2 + 2 * jp + 1];
          const float p0 = __builtin_amdgcn_exp2f(fmaf(x0, scale_log2e, -m_safe));
          const float p1 = __builtin_amdgcn_exp2f(fmaf(x1, scale_log2e, -m_safe));
          w[jp] = pack2<T>(p0, p1);
          psum += p0 + p1;  // row sum from the fp32 probabilities, P itself rounded to the model dtype
        }
        pf[kb2 * 2 + s2] = __builtin_bit_cast(s16x8, make_uint4(w[0], w[1], w[2], w[3]));
      }
    }
    l_run = l_run * alpha + psum;

    // ---- O^T += V(t)^T P(t)^T ------------------------------------------------------------------------------------
    uint32_t va = lds0 + 2 * MXP_KTILE + vcur * MXP_VTILE + v_lane;
    asm volatile("" : "+v"(va));
    const lds_char* vb = (const lds_char*)(uintptr_t)va;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        const uint32_t a0 = ((ks >> 1) * 32 + (ks & 1) * 16) * MXP_VSTR + 64 * db;  // immediate
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb + a0));
        const s16x4 hi =
            __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb + a0 + 8 * MXP_VSTR));
        const s16x8 a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        oacc[db] = mfma32<T>(a, pf[ks], oacc[db]);
      }
    }
    mx_raw = tile_max(sn0, sn1);  // next tile, unmasked; overlaps the PV MFMAs above
    if (t + 2 < ntiles) lstore(t + 2, t & 1, vnext2);
    lds_barrier();
    sc0 = sn0;
    sc1 = sn1;
    vcur = vcur == 2 ? 0 : vcur + 1;
  }

  // ---- epilogue: normalise, stage O through LDS (wave-private region), store whole rows ------------------------
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
  char* ob = smem + wave * (32 * MXP_OSTRIDE);
#pragma unroll
  for (int db = 0; db < DB; ++db) {
#pragma unroll
    for (int i4 = 0; i4 < 4; ++i4) {
      const int d = db * 32 + 8 * i4 + 4 * h;  // accumulator rows (i&3)+8*(i>>2)+4h for i = 4*i4 .. 4*i4+3
      const uint32_t w0 = pack2<T>(oacc[db][4 * i4] * inv, oacc[db][4 * i4 + 1] * inv);
      const uint32_t w1 = pack2<T>(oacc[db][4 * i4 + 2] * inv, oacc[db][4 * i4 + 3] * inv);
      *reinterpret_cast<uint2*>(ob + r * MXP_OSTRIDE + d * 2) = make_uint2(w0, w1);
    }
  }
  // the wave re-reads only what it wrote itself: LDS ops of one wave execute in order, no barrier needed
  constexpr int RPI = 64 / CH;          // rows per store instruction
#pragma unroll
  for (int it = 0; it < 32 / RPI; ++it) {
    const int rr = it * RPI + lane / CH;
    const int ch = lane % CH;
    const int grow = wave * 32 + rr;
    const int ghead = g * G + grow / BM;
    const int gtok = m0 + grow % BM;
    if (gtok < La) {
      const uint4 val = *reinterpret_cast<const uint4*>(ob + rr * MXP_OSTRIDE + ch * 16);
      *reinterpret_cast<uint4*>(out + ((size_t)(s0 + gtok) * HQ + ghead) * D + ch * 8) = val;
    }
  }
}

template <typename T, int D>
static int launch_prefill_mxfp4(int G, const void* q, const void* k, const void* v, int64_t sq_n, int64_t sk_n,
                                int64_t sk_h, int64_t sv_n, int64_t sv_h, const void* kc, const void* vc,
                                const uint8_t* ksc, const uint8_t* vsc, void* out, const int* seq_lens,
                                const int* page_table, const int* bmap, const int* cu, int B, int max_seqlen_q, int HKV,
                                int PS, int NLP, float scale, hipStream_t st) {
#define MXP_CALL(G_)                                                                                                  \
  {                                                                                                                   \
    auto kern = prefill_attn_mxfp4_kernel<T, D, G_>;                                                                  \
    set_dyn_lds_once(kern, MXP_SMEM);                                                                                 \
    const int nqt = (max_seqlen_q + MXP_ROWS / G_ - 1) / (MXP_ROWS / G_);                                             \
    hipLaunchKernelGGL(kern, dim3(nqt* B* HKV), dim3(MXP_THREADS), MXP_SMEM, st, (const uint16_t*)q,                  \
                       (const uint16_t*)k, (const uint16_t*)v, sq_n, sk_n, sk_h, sv_n, sv_h, (const uint8_t*)kc,      \
                       (const uint8_t*)vc, ksc, vsc, (uint16_t*)out, seq_lens, page_table, bmap, cu, B, HKV, PS, NLP, \
                       scale * 1.4426950408889634f);                                                                  \
    return check_launch();                                                                                            \
  }
  switch (G) {
    case 1: MXP_CALL(1);
    case 2: MXP_CALL(2);
    case 4: MXP_CALL(4);
    case 8: MXP_CALL(8);
    default: return CVLLM_ERR_SHAPE;
  }
#undef MXP_CALL
}

}  // namespace cvllm

using namespace cvllm;

extern "C" int cvllm_prefill_attn_mxfp4(const void* q, const void* k, const void* v, int64_t sq_n, int64_t sk_n,
                                        int64_t sk_h, int64_t sv_n, int64_t sv_h, const void* k_cache,
                                        const void* v_cache, void* out, const int32_t* seq_lens_bh,
                                        const int32_t* page_table, const int32_t* batch_mapping,
                                        const int32_t* cu_seqlens_q, int B, int total_tokens, int max_seqlen_q, int HQ,
                                        int HKV, int D, int page_size, int n_logical_pages_max, float sm_scale,
                                        int dtype, cvllm_stream_t stream, const uint8_t* k_scale,
                                        const uint8_t* v_scale) {
  if (!q || !k || !v || !k_cache || !v_cache || !out || !seq_lens_bh || !page_table || !batch_mapping ||
      !cu_seqlens_q || !k_scale || !v_scale)
    return CVLLM_ERR_ARG;
  if (B <= 0 || total_tokens < 0 || HQ <= 0 || HKV <= 0 || page_size <= 0 || n_logical_pages_max <= 0)
    return CVLLM_ERR_ARG;
  if (HQ % HKV != 0) return CVLLM_ERR_SHAPE;
  const int G = HQ / HKV;
  if (G != 1 && G != 2 && G != 4 && G != 8) return CVLLM_ERR_SHAPE;
  if ((D != 64 && D != 128) || (dtype != CVLLM_F16 && dtype != CVLLM_BF16)) return CVLLM_ERR_SHAPE;
  // 16-byte vector loads: every row start must be 16-byte aligned
  if ((sq_n % 8) || (sk_n % 8) || (sk_h % 8) || (sv_n % 8) || (sv_h % 8)) return CVLLM_ERR_SHAPE;
  if (sk_n < 0 || sv_n < 0 || sk_n > 0x7fffffff || sv_n > 0x7fffffff) return CVLLM_ERR_SHAPE;  // 32-bit row strides in the kernel
  if (total_tokens == 0 || max_seqlen_q <= 0) return CVLLM_OK;
  hipStream_t st = (hipStream_t)stream;
#define MXP_D(T_, D_)                                                                                                    \
  return launch_prefill_mxfp4<T_, D_>(G, q, k, v, sq_n, sk_n, sk_h, sv_n, sv_h, k_cache, v_cache, k_scale, v_scale, out, \
                                      seq_lens_bh, page_table, batch_mapping, cu_seqlens_q, B, max_seqlen_q, HKV,        \
                                      page_size, n_logical_pages_max, sm_scale, st)
  if (dtype == CVLLM_F16) {
    if (D == 128) MXP_D(F16, 128);
    MXP_D(F16, 64);
  }
  if (D == 128) MXP_D(BF16, 128);
  MXP_D(BF16, 64);
#undef MXP_D
}
