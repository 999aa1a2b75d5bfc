// Causal varlen prefill attention over [FP8 (e4m3) paged per-head prefix || 16-bit appended block], GQA, gfx950 MFMA.
//
// What chunked prefill and prefix reuse need on an FP8 cache (DESIGN.md sections 2 and 3.2.1): the cached prefix is e4m3
// codes + one fp32 scale per row (kv_fp8.hip), the appended block is the model's 16-bit k / v as in prefill_attn.hip.
//
// Structure: the compiler-scheduled 8-wave kernel of prefill_attn.hip - a workgroup = 256 query rows = (256/G tokens) x G
// heads of one kv-head, 64-key tiles (cached tiles first, then appended tiles up to the diagonal), S^T = K Q^T and
// O^T += V^T P^T with v_mfma_f32_32x32x16, V^T by ds_read_b64_tr_b16, K double- and V triple-buffered padded 16-bit LDS
// images, one barrier per tile, the in-wave software pipeline, exp2-domain online softmax with the deferred rescale.  The
// tile loop is that kernel's, line for line: it carries no scale and no conversion.
//
// What is new is the STAGING.  The FP8 rows are dequantised once per tile, while they are staged, not at fragment-read
// time and not on the logits (the loop is bound by VALU issue; instruction counts in DESIGN.md section 3.2.1):
//   * cached tile: thread (row = tid / 8, 16-code chunk = tid % 8) loads 16 B of K codes and 16 B of V codes of ONE row and
//     that row's two scales - 16 KiB of codes per tile for 512 threads, half the global bytes and half the staging
//     registers of a 16-bit tile - forms rne_T(float(code) * scale) (v_cvt_pk_f32_fp8: exact; one fp32 multiply; one
//     packed RNE conversion to the model dtype T) and writes 2 x 16 B per operand into the SAME padded images;
//   * appended tile: the 16-bit kernel's mapping (rows r, r + 32; 16 B chunk), copied through.
// Both kinds go through the same registers and the same software pipeline (global loads of tile t + 2 at the top of
// iteration t, its LDS writes at the end); which kind a staged tile is, is workgroup-uniform (t < ntc).
//
// Read-back rule of prefill: rne_T(fp32(code) * scale) - one rounding to 16 bit more than the decode kernel's exact fp32
// value; |value| <= the row's original amax, so f16 cannot overflow on rows stored from f16.
//
// Paging and ragged ends are the 16-bit kernel's: the scalar incremental page walk when PS % 64 == 0, a per-row lookup
// otherwise; rows past the end of a tile are CLAMPED to the tile's last valid row (their logits are masked to -inf), so a
// cache row beyond a head's length - any byte, any scale, NaN included - is never read.
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

constexpr int F8P_THR = 8;       // rescale threshold, exp2 domain (PF_THR)
constexpr int F8P_ROWS = 256;    // query rows per workgroup
constexpr int F8P_KT = 64;       // keys per tile
constexpr int F8P_THREADS = 512;
constexpr int F8P_KSTR = 272;    // K image row stride: 256 + 16 B pad -> conflict-free ds_read_b128
constexpr int F8P_VSTR = 320;    // V image row stride: 256 + 64 B pad -> conflict-free ds_read_b64_tr_b16
constexpr int F8P_KTILE = F8P_KT * F8P_KSTR;
constexpr int F8P_VTILE = F8P_KT * F8P_VSTR;
constexpr int F8P_OSTRIDE = 272;
constexpr int F8P_SMEM = 2 * F8P_KTILE + 3 * F8P_VTILE;  // 96,256 B
static_assert(F8P_SMEM >= 8 * 32 * F8P_OSTRIDE, "O staging image must fit");

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

// ---- 16 e4m3 codes of one row -> 16 values of the model dtype, rne_T(float(code) * scale), 2 x 16 B into an LDS image ----
// v_cvt_pk_f32_fp8 is exact (every e4m3 value is an fp32 value); the multiply is a plain fp32 v_mul (v_cvt_scalef32_pk_*
// is NOT used with the row scale: whether it applies more than the scale's exponent is not established here, and the
// decode kernel only ever passes 1.0).
typedef __attribute__((ext_vector_type(2))) float f32x2_v;
template <typename T>
__device__ __forceinline__ void dequant16_to_lds(const u32x4& c, float scale, char* dst) {
  const uint32_t w[4] = {c[0], c[1], c[2], c[3]};
  uint32_t o[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2_v lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f32x2_v hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    o[2 * i] = pack2<T>(lo[0] * scale, lo[1] * scale);
    o[2 * i + 1] = pack2<T>(hi[0] * scale, hi[1] * scale);
  }
  *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
  *reinterpret_cast<uint4*>(dst + 16) = make_uint4(o[4], o[5], o[6], o[7]);
}

template <typename T, int D, int G>
__global__ __launch_bounds__(F8P_THREADS) void prefill_attn_fp8_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, int64_t sq_n,
    int64_t sk_n, int64_t sk_h, int64_t sv_n, int64_t sv_h, const uint8_t* __restrict__ kc,
    const uint8_t* __restrict__ vc, const float* __restrict__ ksc, const float* __restrict__ vsc,
    uint16_t* __restrict__ out, const int* __restrict__ seq_lens, const int* __restrict__ page_table,
    const int* __restrict__ bmap, const int* __restrict__ cu, int B, int HKV, int PS, int NLP, float scale_log2e) {
  constexpr int BM = F8P_ROWS / G;  // tokens per query tile
  constexpr int KS = D / 16;        // k-steps of the QK^T product
  constexpr int DB = D / 32;        // 32-wide blocks of the head dim
  constexpr int CH = D / 8;         // 16-byte chunks per 16-bit row
  constexpr int CH8 = D / 16;       // 16-byte chunks per row of codes

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

  const int ntc = (Lc + F8P_KT - 1) / F8P_KT;                     // cached-prefix tiles (FP8)
  const int la_vis = min(m0 + BM, La);                            // appended keys visible to this query tile
  const int nta = (la_vis + F8P_KT - 1) / F8P_KT;                 // appended tiles (16 bit; the last ones are on the diagonal)
  const int ntiles = ntc + nta;

  // ---- staging ---------------------------------------------------------------------------------------------------------
  // appended (16-bit) tile: thread -> (rows srow, srow + 32; 16 B chunk sch), four registers kr0 kr1 vr0 vr1
  // cached (FP8) tile:      thread -> (row fr; 16-code chunk fc): kr0 = K codes, vr0 = V codes, ksr / vsr = the row's scales
  const int sch = tid & 15;
  const int srow = tid >> 4;  // 0..31
  const bool stage_active = sch < CH;
  u32x4 kr0, kr1, vr0, vr1;  // named scalars (arrays captured by the lambdas go to scratch)
  float ksr = 0.f, vsr = 0.f;
  // Beyond the two scales the FP8 mapping keeps NO register live across the MFMA loop (the 16-bit kernel sits at the
  // 256-register limit already): its lane constants are recomputed from a laundered copy of tid where they are used (a
  // handful of VALU per tile) and the loads are uniform base + 32-bit lane offset.  A cached tile leaves kr1 / vr1 unused
  // and says so (f8_kill): carried through as live values they make hipcc land the appended tiles' loads in other registers
  // and copy them over behind a vmcnt(0) at the top of the iteration.
  auto f8_kill = [&]() { asm volatile("" : "=v"(kr1), "=v"(vr1)); };
  auto f8_lane = [&](int& fr, int& fc) {
    int tl = tid;
    asm volatile("" : "+v"(tl));
    fr = tl >> 3;  // row of the tile, 0..63
    fc = tl & 7;   // 16-code chunk of the row; active if < CH8
  };

  // Rows past the end of a tile are clamped to its last valid row, never skipped and never read from beyond the head's
  // length: their logits are masked to -inf (P = 0) and the clamped row is finite data, so 0 * V stays 0.
  const bool ps64 = (PS % F8P_KT) == 0;
  int ld_pi = 0, ld_po = 0;                 // page index / offset in page of the next cached tile to load
  int ld_pg = (ntc > 0) ? pt[0] : 0;        // its physical page
  const uint32_t skn = (uint32_t)sk_n, svn = (uint32_t)sv_n;  // row strides < 2^31 elements (checked on the host)
  auto gload = [&](int t) {
    if (t < ntc) {
      int fr, fc;
      f8_lane(fr, fc);
      size_t base;   // physical cache row (index of the codes' row AND of its scales): workgroup-uniform part
      uint32_t rl;   // ... and the lane's part
      if (ps64) {
        base = (size_t)ld_pg * PS + ld_po;
        rl = (uint32_t)min(fr, Lc - 1 - t * F8P_KT);  // last valid row of the tile, >= 0
        ld_po += F8P_KT;
        if (ld_po >= PS) {
          ld_po = 0;
          ld_pi += 1;
          ld_pg = pt[min(ld_pi, NLP - 1)];
        }
      } else {
        const int p = min(t * F8P_KT + fr, Lc - 1);
        base = (size_t)pt[p / PS] * PS + p % PS;
        rl = 0;
      }
      f8_kill();
      if (fc < CH8) {
        const uint32_t off = rl * D + fc * 16;
        kr0 = *reinterpret_cast<const u32x4*>(kc + base * D + off);
        vr0 = *reinterpret_cast<const u32x4*>(vc + base * D + off);
        ksr = (ksc + base)[rl];
        vsr = (vsc + base)[rl];
      }
    } else if (stage_active) {
      const uint32_t n0 = (uint32_t)(s0 + min((t - ntc) * F8P_KT + srow, la_vis - 1));
      const uint32_t n1 = (uint32_t)(s0 + min((t - ntc) * F8P_KT + srow + 32, la_vis - 1));
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
  char* const vbase = smem + 2 * F8P_KTILE;
  const uint32_t kst = srow * F8P_KSTR + sch * 16, vst = srow * F8P_VSTR + sch * 16;
  // tile t (the one the staging registers hold) -> K buffer kbuf, V buffer vbuf
  auto lstore = [&](int t, int kbuf, int vbuf) {
    if (t < ntc) {
      int fr, fc;
      f8_lane(fr, fc);
      if (fc < CH8) {
        dequant16_to_lds<T>(kr0, ksr, kbase + kbuf * F8P_KTILE + fr * F8P_KSTR + fc * 32);
        dequant16_to_lds<T>(vr0, vsr, vbase + vbuf * F8P_VTILE + fr * F8P_VSTR + fc * 32);
      }
    } else if (stage_active) {
      char* kb = kbase + kbuf * F8P_KTILE + kst;
      char* vb = vbase + vbuf * F8P_VTILE + vst;
      *reinterpret_cast<u32x4*>(kb) = kr0;
      *reinterpret_cast<u32x4*>(kb + 32 * F8P_KSTR) = kr1;
      *reinterpret_cast<u32x4*>(vb) = vr0;
      *reinterpret_cast<u32x4*>(vb + 32 * F8P_VSTR) = vr1;
    }
  };
  const uint32_t k_lane = r * F8P_KSTR + h * 16;                                           // + 32 s (+ 32 rows)
  const uint32_t v_lane = (4 * (gi >> 1) + tq) * F8P_VSTR + (gi & 1) * 32 + tp * 8;       // + rows, + 64 db
  typedef __attribute__((address_space(3))) char lds_char;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_char*)smem;  // LDS byte address of the dynamic segment
  // tile base added to the lane constant ONCE and laundered: every read is that VGPR plus an immediate
  auto qk_tile = [&](int kbuf, f32x16& s0_, f32x16& s1_) {
    uint32_t ka = lds0 + kbuf * F8P_KTILE + k_lane;
    asm volatile("" : "+v"(ka));
    const lds_char* kb = (const lds_char*)(uintptr_t)ka;
#pragma unroll
    for (int i = 0; i < 16; ++i) s0_[i] = 0.f, s1_[i] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const s16x8 a0 = *reinterpret_cast<const __attribute__((address_space(3))) s16x8*>(kb + 32 * s);
      const s16x8 a1 = *reinterpret_cast<const __attribute__((address_space(3))) s16x8*>(kb + 32 * s + 32 * F8P_KSTR);
      s0_ = mfma32<T>(a0, qf[s], s0_);
      s1_ = mfma32<T>(a1, qf[s], s1_);
    }
  };

  // ---- main loop: prefill_attn_kernel's, one 64-key tile per iteration, software-pipelined by one tile -------------------
  // K(t+2) replaces K(t) (last read in iteration t-1), V(t+2) replaces V(t-1); global loads of tile t+2 at the top of
  // iteration t, its LDS writes - with the dequantisation, if it is a cached tile - at the end, behind ONE barrier per tile.
  // The switch from 1-byte to 2-byte staging happens between two tiles of this pipeline: gload(t) and lstore(t, ..) decide
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
    const int j0 = cached ? t * F8P_KT : (t - ntc) * F8P_KT;
    const int count = cached ? min(F8P_KT, Lc - j0) : min(F8P_KT, la_vis - j0);
    const bool need_mask = count < F8P_KT || (!cached && j0 + F8P_KT - 1 > m0);  // wave-uniform
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
    // deferred rescale: the running max follows the row max only once it has grown by more than F8P_THR (exp2 domain)
    const bool grew = mx > m_run + (float)F8P_THR;
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
    uint32_t va = lds0 + 2 * F8P_KTILE + vcur * F8P_VTILE + v_lane;
    asm volatile("" : "+v"(va));
    const lds_char* vb = (const lds_char*)(uintptr_t)va;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        const uint32_t a0 = ((ks >> 1) * 32 + (ks & 1) * 16) * F8P_VSTR + 64 * db;  // immediate
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb + a0));
        const s16x4 hi =
            __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb + a0 + 8 * F8P_VSTR));
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
  char* ob = smem + wave * (32 * F8P_OSTRIDE);
#pragma unroll
  for (int db = 0; db < DB; ++db) {
#pragma unroll
    for (int i4 = 0; i4 < 4; ++i4) {
      const int d = db * 32 + 8 * i4 + 4 * h;  // accumulator rows (i&3)+8*(i>>2)+4h for i = 4*i4 .. 4*i4+3
      const uint32_t w0 = pack2<T>(oacc[db][4 * i4] * inv, oacc[db][4 * i4 + 1] * inv);
      const uint32_t w1 = pack2<T>(oacc[db][4 * i4 + 2] * inv, oacc[db][4 * i4 + 3] * inv);
      *reinterpret_cast<uint2*>(ob + r * F8P_OSTRIDE + d * 2) = make_uint2(w0, w1);
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
      const uint4 val = *reinterpret_cast<const uint4*>(ob + rr * F8P_OSTRIDE + ch * 16);
      *reinterpret_cast<uint4*>(out + ((size_t)(s0 + gtok) * HQ + ghead) * D + ch * 8) = val;
    }
  }
}

template <typename T, int D>
static int launch_prefill_fp8(int G, const void* q, const void* k, const void* v, int64_t sq_n, int64_t sk_n,
                              int64_t sk_h, int64_t sv_n, int64_t sv_h, const void* kc, const void* vc,
                              const float* ksc, const float* vsc, void* out, const int* seq_lens,
                              const int* page_table, const int* bmap, const int* cu, int B, int max_seqlen_q, int HKV,
                              int PS, int NLP, float scale, hipStream_t st) {
#define F8P_CALL(G_)                                                                                                  \
  {                                                                                                                   \
    auto kern = prefill_attn_fp8_kernel<T, D, G_>;                                                                    \
    set_dyn_lds_once(kern, F8P_SMEM);                                                                                 \
    const int nqt = (max_seqlen_q + F8P_ROWS / G_ - 1) / (F8P_ROWS / G_);                                             \
    hipLaunchKernelGGL(kern, dim3(nqt* B* HKV), dim3(F8P_THREADS), F8P_SMEM, st, (const uint16_t*)q,                  \
                       (const uint16_t*)k, (const uint16_t*)v, sq_n, sk_n, sk_h, sv_n, sv_h, (const uint8_t*)kc,      \
                       (const uint8_t*)vc, ksc, vsc, (uint16_t*)out, seq_lens, page_table, bmap, cu, B, HKV, PS, NLP, \
                       scale * 1.4426950408889634f);                                                                  \
    return check_launch();                                                                                            \
  }
  switch (G) {
    case 1: F8P_CALL(1);
    case 2: F8P_CALL(2);
    case 4: F8P_CALL(4);
    case 8: F8P_CALL(8);
    default: return CVLLM_ERR_SHAPE;
  }
#undef F8P_CALL
}

}  // namespace cvllm

using namespace cvllm;

extern "C" int cvllm_prefill_attn_fp8(const void* q, const void* k, const void* v, int64_t sq_n, int64_t sk_n,
                                      int64_t sk_h, int64_t sv_n, int64_t sv_h, const void* k_cache,
                                      const void* v_cache, void* out, const int32_t* seq_lens_bh,
                                      const int32_t* page_table, const int32_t* batch_mapping,
                                      const int32_t* cu_seqlens_q, int B, int total_tokens, int max_seqlen_q, int HQ,
                                      int HKV, int D, int page_size, int n_logical_pages_max, float sm_scale, int dtype,
                                      cvllm_stream_t stream, const float* k_scale, const float* v_scale) {
  if (!q || !k || !v || !k_cache || !v_cache || !out || !seq_lens_bh || !page_table || !batch_mapping ||
      !cu_seqlens_q || !k_scale || !v_scale)
    return CVLLM_ERR_ARG;
  if (B <= 0 || total_tokens < 0 || HQ <= 0 || HKV <= 0 || page_size <= 0 || n_logical_pages_max <= 0)
    return CVLLM_ERR_ARG;
  if (HQ % HKV != 0) return CVLLM_ERR_SHAPE;
  if (total_tokens == 0 || max_seqlen_q <= 0) return CVLLM_OK;
  // 16-byte vector loads: every row start must be 16-byte aligned
  if ((sq_n % 8) || (sk_n % 8) || (sk_h % 8) || (sv_n % 8) || (sv_h % 8)) return CVLLM_ERR_SHAPE;
  if (sk_n < 0 || sv_n < 0 || sk_n > 0x7fffffff || sv_n > 0x7fffffff) return CVLLM_ERR_SHAPE;  // 32-bit row strides in the kernel
  const int G = HQ / HKV;
  hipStream_t st = (hipStream_t)stream;
#define F8P_D(T_, D_)                                                                                                 \
  return launch_prefill_fp8<T_, D_>(G, q, k, v, sq_n, sk_n, sk_h, sv_n, sv_h, k_cache, v_cache, k_scale, v_scale, out, \
                                    seq_lens_bh, page_table, batch_mapping, cu_seqlens_q, B, max_seqlen_q, HKV,        \
                                    page_size, n_logical_pages_max, sm_scale, st)
  if (dtype == CVLLM_F16) {
    if (D == 128) F8P_D(F16, 128);
    if (D == 64) F8P_D(F16, 64);
  } else if (dtype == CVLLM_BF16) {
    if (D == 128) F8P_D(BF16, 128);
    if (D == 64) F8P_D(BF16, 64);
  }
#undef F8P_D
  return CVLLM_ERR_SHAPE;
}
