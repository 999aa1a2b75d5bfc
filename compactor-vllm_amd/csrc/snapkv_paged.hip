// SnapKV window scores with the keys read in place: [paged cache prefix (16 bit or FP8 e4m3) || packed chunk], gfx950 MFMA.
//
// What a chunked prefill and a prefill over a reused prefix need ("SnapKV over the paged cache"):
// SnapKV scores a sequence once, with its last w queries over ALL its keys, and most of those keys are in the layer's
// paged cache by then.  For sequence b and kv-head g, with L = cu_k[b+1] - cu_k[b] and P = L - (cu_new[b+1] - cu_new[b]):
//   key j <  P : row page_table[bmap[b], g, j / PS] * PS + j % PS of k_cache (16-bit elements, or e4m3 codes + k_scale[row])
//   key j >= P : row cu_new[b] + j - P of the packed k
//
// The compute is snapkv_kernel's (scoring.hip), restated line for line: the decomposition (b, kv-head, group of SK_TPW
// tiles of 128 keys), pass 1 / the row-LSE reduce (scoring.hip's snapkv_lse_kernel itself, launch_snapkv_lse) / pass 2,
// the MFMA operand order, the per-block (max, sum) fold, the lane-half merge and the pooling epilogue.  The MFMA loop reads
// the same swizzled 16-bit LDS image of a key tile whatever the tile's source, so the scores equal, bit for bit,
// cvllm_snapkv_scores_wb on the gathered (and, for FP8, read-back) keys.
//
// What is new is how a key tile reaches that image:
//   * page ids once per workgroup: a workgroup covers at most 512 consecutive keys; the page ids of their cached part are
//     the FIRST loads the workgroup issues (ahead of the Q fragments: loads return in issue order), then parked in LDS.
//     The tile loop never loads from the page table.
//   * every tile has a workgroup-uniform kind, decided once per tile from (P, L - w):
//       cache  - all scored rows of the tile are cached.  With PS % 128 == 0 the tile sits inside one page: one page id
//                from LDS made scalar, then 32 KiB (16 bit) / 16 KiB + 512 B of scales (FP8) of contiguous rows at a
//                uniform base + lane offset.  Other page sizes look every row's page up in LDS.
//       packed - the 16-bit kernel's loads.
//       seam   - the one tile of a sequence that contains P: the source is a per-row select.
//   * an FP8 tile stays codes in flight: thread (row, 16-code chunk c) keeps 16 B of codes and the row's scale in the
//     register ring - half the ring of a 16-bit tile - and dequantises at the LDS store, rne_T(fp32(code) * scale)
//     (v_cvt_pk_f32_fp8: exact; one fp32 multiply; one packed RNE conversion: prefill_fp8.hip's read-back rule and
//     instruction sequence), into the two 16-byte chunks 2c, 2c + 1 of the row.  An FP8 seam tile keeps the 16-bit
//     mapping: a cached row's thread holds 8 codes and the scale inside its one 16-byte ring entry.
//   * never read: a cache row at or past min(P, L - w) and a packed row at or past L - w.  Their image rows are zeros (a
//     stale FP8 row may hold NaN codes under a NaN scale; rows [L - w, L) are masked as in the 16-bit kernel).
#include "common.h"

namespace cvllm {

// ---- snapkv_kernel's helpers and constants (scoring.hip; same definitions) -------------------------------------------
template <typename T>
__device__ __forceinline__ f32x16 skp_mfma(s16x8 a, s16x8 b, f32x16 c);
template <>
__device__ __forceinline__ f32x16 skp_mfma<F16>(s16x8 a, s16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x16 skp_mfma<BF16>(s16x8 a, s16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
                                                 0);
}
// K tile in LDS: row-major, 16-byte chunks XOR-swizzled by the row
__device__ __forceinline__ uint32_t skp_off(int row, int ch) { return row * 256 + 16 * (ch ^ (row & 15)); }
__device__ __forceinline__ float skp_max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
constexpr int SKP_TILE = 128;
constexpr int SKP_MAXQB = 8;
constexpr int SKP_TPW = 4;
constexpr int SKP_TILE_BYTES = SKP_TILE * 256;
// page ids of one workgroup's keys: 512 keys touch at most 512 pages (PS = 1) / 512 / PS + 2 pages (unaligned PS)
constexpr int SKP_MAXPG = SKP_TPW * SKP_TILE + 2;
constexpr size_t SKP_SMEM = 2 * SKP_TILE_BYTES + 4 * SKP_TPW * SKP_TILE * sizeof(float) + SKP_MAXQB * 32 * sizeof(float) +
                            SKP_MAXPG * sizeof(int);

// 8 e4m3 codes (two words) -> 8 values of T, rne_T(float(code) * scale): prefill_fp8.hip's dequant16_to_lds, one chunk
typedef __attribute__((ext_vector_type(2))) float skp_f32x2;
template <typename T>
__device__ __forceinline__ uint4 skp_dequant8(uint32_t w0, uint32_t w1, float scale) {
  const skp_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
  const skp_f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
  return make_uint4(pack2<T>(a[0] * scale, a[1] * scale), pack2<T>(b[0] * scale, b[1] * scale),
                    pack2<T>(c[0] * scale, c[1] * scale), pack2<T>(d[0] * scale, d[1] * scale));
}

enum { SKP_CACHE = 0, SKP_PACKED = 1, SKP_SEAM = 2 };

// NJQ = 32-row query blocks per wave (1: w*G <= 128, 2: up to 256); F8: k_cache holds e4m3 codes, ksc the row scales
template <typename T, int D, int G, int NJQ, bool PASS2, bool F8>
__global__ __launch_bounds__(256, 2) void snapkv_paged_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, int64_t sq_n, int64_t sk_n, int64_t sk_h,
    const uint8_t* __restrict__ kc, const float* __restrict__ ksc, const int* __restrict__ page_table,
    const int* __restrict__ bmap, float* __restrict__ scores, float* __restrict__ part, const float* __restrict__ lse,
    const int* __restrict__ cu_q, const int* __restrict__ cu_new, const int* __restrict__ cu_k, int B, int HKV, int w_max,
    const int* __restrict__ w_b, int ntile_max, float scale_log2e, int pool, int pool_tile, int PS, int NLP) {
  constexpr int KS = D / 16;
  constexpr int CH = D / 8;                // 16-byte chunks of a 16-bit row
  constexpr int CH8 = D / 16;              // 16-byte chunks of a row of codes
  constexpr int KPT = SKP_TILE * CH / 256;   // 16-byte chunks of a 16-bit K tile per thread
  constexpr int KPT8 = SKP_TILE * CH8 / 256; // ... of a tile of codes
  constexpr int ES = F8 ? 1 : 2;           // bytes per cache element
  constexpr int PF = NJQ == 1 ? 2 : 1;     // K tiles in flight in registers behind the one being staged
  extern __shared__ __attribute__((aligned(16))) char skp_smem[];
  char* s_k = skp_smem;                                                       // [2][SKP_TILE_BYTES]
  float* s_col = reinterpret_cast<float*>(skp_smem + 2 * SKP_TILE_BYTES);     // [4 waves][SKP_TPW * SKP_TILE]
  float* s_lse = s_col + 4 * SKP_TPW * SKP_TILE;                              // [SKP_MAXQB * 32]
  int* s_pg = reinterpret_cast<int*>(s_lse + SKP_MAXQB * 32);                 // [SKP_MAXPG]

  const int ngrp_max = (ntile_max + SKP_TPW - 1) / SKP_TPW;
  const int bid = blockIdx.x;
  const int g = bid % HKV;
  const int grp = (bid / HKV) % ngrp_max;
  const int b = bid / (HKV * ngrp_max);
  const int kb0 = cu_k[b], Lk = cu_k[b + 1] - kb0;
  const int nb0 = cu_new[b];
  const int P = max(0, Lk - (cu_new[b + 1] - nb0));  // cached prefix
  const int qend = cu_q[b + 1];
  const int w = min(w_b ? w_b[b] : w_max, w_max);
  const int keff = Lk - w;  // keys that are scored
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  if (w <= 0) {
    if (PASS2 && grp == 0)
      for (int i = tid; i < Lk; i += 256) scores[(size_t)(kb0 + i) * HKV + g] = 0.f;
    return;
  }
  if (keff <= 0) {
    if (PASS2 && grp == 0)
      for (int i = tid; i < Lk; i += 256) scores[(size_t)(kb0 + i) * HKV + g] = INFINITY;
    return;
  }
  const int ntile = (keff + SKP_TILE - 1) / SKP_TILE;
  const int tile0 = grp * SKP_TPW, tile1 = min(ntile, tile0 + SKP_TPW);
  if (tile0 >= ntile) return;
  const int rows_b = w * G;
  const int nqb = (rows_b + 31) / 32;

  // ---- page ids of this workgroup's cached keys [tile0 * 128, jc1): the first loads issued -----------------------------
  const int pc = min(P, keff);                      // cached keys that are scored: the only cache rows ever read
  const int jc1 = min(pc, tile1 * SKP_TILE);
  const int pg0 = tile0 * SKP_TILE / PS;
  const int npg = jc1 > tile0 * SKP_TILE ? (jc1 - 1) / PS - pg0 + 1 : 0;  // <= SKP_MAXPG
  const int* pt = page_table + ((size_t)bmap[b] * HKV + g) * NLP;
  int pgv[3];
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int i = tid + 256 * u;
    pgv[u] = i < npg ? pt[min(pg0 + i, NLP - 1)] : 0;
  }

  // ---- tile sourcing -----------------------------------------------------------------------------------------------------
  const bool pg_al = (PS & (SKP_TILE - 1)) == 0;  // a tile never crosses a page
  auto kind = [&](int tile) {                     // workgroup-uniform
    const int t0 = tile * SKP_TILE;
    return pc >= min(t0 + SKP_TILE, keff) ? SKP_CACHE : pc <= t0 ? SKP_PACKED : SKP_SEAM;
  };
  auto crow = [&](int j) -> size_t { return (size_t)s_pg[j / PS - pg0] * PS + j % PS; };  // cache row of key j < jc1
  auto prow = [&](int j) { return k + (size_t)(nb0 + j - P) * sk_n + (size_t)g * sk_h; };  // packed row of key j >= P

  uint4 kreg[PF][KPT];  // register ring; every index is a constant once the tile loop is unrolled
  float kscl[PF][KPT8]; // FP8 cache tiles: kreg[slot][0 .. KPT8) are codes, kscl their rows' scales
  auto gload = [&](int slot, int tile) {
    const int t0 = tile * SKP_TILE, M = min(SKP_TILE, keff - t0);
    const int kd = kind(tile);
    if (kd == SKP_PACKED) {
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        const int e = tid + 256 * j, row = e / CH, ch = e % CH;
        kreg[slot][j] = make_uint4(0, 0, 0, 0);
        if (row < M) kreg[slot][j] = *reinterpret_cast<const uint4*>(prow(t0 + row) + ch * 8);
      }
    } else if (kd == SKP_CACHE && (F8 || pg_al)) {
      // whole-page tile: ONE page id, scalar; the tile's rows are contiguous behind it
      const size_t ubase =
          pg_al ? (size_t)__builtin_amdgcn_readfirstlane(s_pg[t0 / PS - pg0]) * PS + t0 % PS : 0;
      if (F8) {
#pragma unroll
        for (int j = 0; j < KPT8; ++j) {
          const int e = tid + 256 * j, row = e / CH8, c = e % CH8;
          kreg[slot][j] = make_uint4(0, 0, 0, 0);
          kscl[slot][j] = 0.f;
          if (row < M) {
            const size_t pr = pg_al ? ubase + row : crow(t0 + row);
            kreg[slot][j] = *reinterpret_cast<const uint4*>(kc + pr * D + c * 16);
            kscl[slot][j] = ksc[pr];
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
          const int e = tid + 256 * j, row = e / CH, ch = e % CH;
          kreg[slot][j] = make_uint4(0, 0, 0, 0);
          if (row < M) kreg[slot][j] = *reinterpret_cast<const uint4*>(kc + ((ubase + row) * D + ch * 8) * ES);
        }
      }
    } else {
      // per-row select: the seam tile, and 16-bit cache tiles of a page size that is no multiple of 128
      const int nc = pc - t0;  // rows [0, nc) are cached, [nc, M) packed
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        const int e = tid + 256 * j, row = e / CH, ch = e % CH;
        kreg[slot][j] = make_uint4(0, 0, 0, 0);
        if (row < nc && row < M) {
          const size_t pr = crow(t0 + row);
          if (F8) {  // 8 codes and the row's scale in one ring entry
            const uint2 c = *reinterpret_cast<const uint2*>(kc + pr * D + ch * 8);
            kreg[slot][j] = make_uint4(c.x, c.y, __float_as_uint(ksc[pr]), 0);
          } else {
            kreg[slot][j] = *reinterpret_cast<const uint4*>(kc + (pr * D + ch * 8) * ES);
          }
        } else if (row < M) {
          kreg[slot][j] = *reinterpret_cast<const uint4*>(prow(t0 + row) + ch * 8);
        }
      }
    }
  };
  auto lstore = [&](int slot, int buf, int tile) {
    char* kb = s_k + buf * SKP_TILE_BYTES;
    const int kd = F8 ? kind(tile) : SKP_PACKED;  // a 16-bit cache's tiles are 16-bit chunks whatever their source
    if (kd == SKP_CACHE) {
#pragma unroll
      for (int j = 0; j < KPT8; ++j) {
        const int e = tid + 256 * j, row = e / CH8, c = e % CH8;
        const uint4 cw = kreg[slot][j];
        *reinterpret_cast<uint4*>(kb + skp_off(row, 2 * c)) = skp_dequant8<T>(cw.x, cw.y, kscl[slot][j]);
        *reinterpret_cast<uint4*>(kb + skp_off(row, 2 * c + 1)) = skp_dequant8<T>(cw.z, cw.w, kscl[slot][j]);
      }
    } else if (kd == SKP_SEAM) {
      const int nc = pc - tile * SKP_TILE;
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        const int e = tid + 256 * j, row = e / CH, ch = e % CH;
        const uint4 cw = kreg[slot][j];
        *reinterpret_cast<uint4*>(kb + skp_off(row, ch)) =
            row < nc ? skp_dequant8<T>(cw.x, cw.y, __uint_as_float(cw.z)) : cw;
      }
    } else {
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        const int e = tid + 256 * j;
        *reinterpret_cast<uint4*>(kb + skp_off(e / CH, e % CH)) = kreg[slot][j];
      }
    }
  };

  // this wave's query blocks (qb = wave, wave + 4): fragments stay in registers for all tiles of the workgroup; issued
  // behind the page ids and BEFORE the K tiles (scoring.hip: with Q behind two K tiles the first MFMA waited 6.7 us)
  s16x8 qf[NJQ][KS];
#pragma unroll
  for (int jq = 0; jq < NJQ; ++jq) {
    const int row = (wave + 4 * jq) * 32 + r;  // window row -> (query offset, local head): row = qoff*G + hq_local
    const bool valid_q = row < rows_b;
    const int qoff = row / G, hql = row % G;
    const uint16_t* qp = q + (size_t)(qend - w + (valid_q ? qoff : 0)) * sq_n + (size_t)(g * G + hql) * D + 8 * h;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      uint4 t = valid_q ? *reinterpret_cast<const uint4*>(qp + 16 * s) : make_uint4(0, 0, 0, 0);
      qf[jq][s] = __builtin_bit_cast(s16x8, t);
    }
  }
  if (PASS2) {
    const float* lp = lse + ((size_t)b * HKV + g) * (SKP_MAXQB * 32);
    for (int row = tid; row < nqb * 32; row += 256) s_lse[row] = row < rows_b ? lp[row] : INFINITY;
  }
  // the page ids have arrived first (the Q fragments stay in flight): parked, then every K address comes from LDS
#pragma unroll
  for (int u = 0; u < 3; ++u)
    if (tid + 256 * u < npg) s_pg[tid + 256 * u] = pgv[u];
  __syncthreads();
#pragma unroll
  for (int p = 0; p < PF; ++p)
    if (tile0 + p < tile1) gload(p, tile0 + p);
  lstore(0, 0, tile0);
  if (tile0 + PF < tile1) gload(0, tile0 + PF);
  __syncthreads();

  // ---- from here on: snapkv_kernel, line for line ------------------------------------------------------------------------
  // pass 1: (max, sum) of this lane's half of the keys, per query block, carried over the group's tiles
  float mx[NJQ], sum[NJQ];
#pragma unroll
  for (int jq = 0; jq < NJQ; ++jq) mx[jq] = -INFINITY, sum[jq] = 0.f;
  // pass 2: -lse of the 16 query rows this lane's accumulators hold (rows past the window: -inf -> weight 0)
  float nlse[NJQ][16];
  if (PASS2) {
#pragma unroll
    for (int jq = 0; jq < NJQ; ++jq)
#pragma unroll
      for (int i = 0; i < 16; ++i) nlse[jq][i] = -s_lse[(wave + 4 * jq) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h];
  }

#pragma unroll
  for (int ti = 0; ti < SKP_TPW; ++ti) {
    const int tile = tile0 + ti;
    if (tile >= tile1) break;  // workgroup-uniform
    const int t0 = tile * SKP_TILE, M = min(SKP_TILE, keff - t0);
    const bool full = M == SKP_TILE;  // only a sequence's last tile needs the key mask
    const char* kt = s_k + (ti & 1) * SKP_TILE_BYTES;
    s16x8 kf[2][KS];
    auto load_kf = [&](int slot, int kb) {
#pragma unroll
      for (int s = 0; s < KS; ++s)
        kf[slot][s] = *reinterpret_cast<const s16x8*>(kt + skp_off(kb * 32 + r, 2 * s + h));
    };
    float colsum[4] = {0.f, 0.f, 0.f, 0.f};
    load_kf(0, 0);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      if (kb < 3) load_kf((kb + 1) & 1, kb + 1);
#pragma unroll
      for (int jq = 0; jq < NJQ; ++jq) {
        if (wave + 4 * jq >= nqb) continue;  // wave-uniform
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        if (!PASS2) {
#pragma unroll
          for (int s = 0; s < KS; ++s) acc = skp_mfma<T>(kf[kb & 1][s], qf[jq][s], acc);
          if (!full) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h < M ? acc[i] : -INFINITY;
          }
          float m0 = skp_max3(acc[0], acc[1], acc[2]), m1 = skp_max3(acc[3], acc[4], acc[5]);
          m0 = skp_max3(m0, acc[6], acc[7]), m1 = skp_max3(m1, acc[8], acc[9]);
          m0 = skp_max3(m0, acc[10], acc[11]), m1 = skp_max3(m1, acc[12], acc[13]);
          const float mb = skp_max3(m0, m1, fmaxf(acc[14], acc[15])) * scale_log2e;
          const float mbs = (!full && mb == -INFINITY) ? 0.f : mb;  // a lane whose 16 keys are all past the end
          float bs0 = 0.f, bs1 = 0.f;
#pragma unroll
          for (int i = 0; i < 16; i += 2) {
            bs0 += __builtin_amdgcn_exp2f(fmaf(acc[i], scale_log2e, -mbs));
            bs1 += __builtin_amdgcn_exp2f(fmaf(acc[i + 1], scale_log2e, -mbs));
          }
          const float mn = fmaxf(mx[jq], mb);
          const float mns = (!full && mn == -INFINITY) ? 0.f : mn;
          sum[jq] = sum[jq] * __builtin_amdgcn_exp2f(mx[jq] - mns) + (bs0 + bs1) * __builtin_amdgcn_exp2f(mb - mns);
          mx[jq] = mn;
        } else {
#pragma unroll
          for (int s = 0; s < KS; ++s) acc = skp_mfma<T>(qf[jq][s], kf[kb & 1][s], acc);
          float c0 = 0.f, c1 = 0.f;
#pragma unroll
          for (int i = 0; i < 16; i += 2) {
            c0 += __builtin_amdgcn_exp2f(fmaf(acc[i], scale_log2e, nlse[jq][i]));
            c1 += __builtin_amdgcn_exp2f(fmaf(acc[i + 1], scale_log2e, nlse[jq][i + 1]));
          }
          colsum[kb] += c0 + c1;
        }
      }
    }
    if (PASS2) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(colsum[kb]), __float_as_uint(colsum[kb]), false, false);
        if (h == 0) s_col[(wave * SKP_TPW + ti) * SKP_TILE + kb * 32 + r] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
      }
    }
    if (tile + 1 < tile1) {
      lstore((ti + 1) % PF, (ti + 1) & 1, tile + 1);
      if (tile + 1 + PF < tile1) gload((ti + 1) % PF, tile + 1 + PF);
    }
    __syncthreads();
  }

  if (!PASS2) {
#pragma unroll
    for (int jq = 0; jq < NJQ; ++jq) {
      const int row = (wave + 4 * jq) * 32 + r;
      const auto sm = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx[jq]), __float_as_uint(mx[jq]), false, false);
      const auto ss = __builtin_amdgcn_permlane32_swap(__float_as_uint(sum[jq]), __float_as_uint(sum[jq]), false, false);
      const float m_lo = __uint_as_float(sm[0]), m_hi = __uint_as_float(sm[1]);
      const float mn = fmaxf(m_lo, m_hi);
      const float tot = __uint_as_float(ss[0]) * __builtin_amdgcn_exp2f(m_lo - mn) +
                        __uint_as_float(ss[1]) * __builtin_amdgcn_exp2f(m_hi - mn);
      if (h == 0 && row < rows_b) {
        float* pp = part + ((((size_t)b * HKV + g) * ngrp_max + grp) * (SKP_MAXQB * 32) + row) * 2;
        pp[0] = mn;
        pp[1] = tot;
      }
    }
  } else {
    const int nk = min(keff - tile0 * SKP_TILE, (tile1 - tile0) * SKP_TILE);
    constexpr int WS = SKP_TPW * SKP_TILE;
    for (int i = tid; i < nk; i += 256) s_col[i] = s_col[i] + s_col[WS + i] + s_col[2 * WS + i] + s_col[3 * WS + i];
    __syncthreads();
    for (int i = tid; i < nk; i += 256) {
      const int j = i & (pool_tile - 1);
      const int lo = max(0, j - (pool - 1));
      float t = 0.f;
      for (int jj = lo; jj <= j; ++jj) t += s_col[i - j + jj];
      scores[(size_t)(kb0 + tile0 * SKP_TILE + i) * HKV + g] = t / (float)(j - lo + 1);
    }
    if (tile0 == 0)
      for (int i = tid; i < w; i += 256) scores[(size_t)(kb0 + keff + i) * HKV + g] = INFINITY;
  }
}

template <typename T, int D, bool F8>
static int snapkv_paged_g(int G, const void* q, const void* k, int64_t sq_n, int64_t sk_n, int64_t sk_h, const void* kc,
                          const float* ksc, const int* page_table, const int* bmap, float* scores, float* part,
                          const int* cu_q, const int* cu_new, const int* cu_k, int B, int HKV, int w, const int* w_b,
                          int ntile, float scale, int pool, int pool_tile, int PS, int NLP, hipStream_t st) {
  const float c = scale * 1.4426950408889634f;
  dim3 grid(B * ((ntile + SKP_TPW - 1) / SKP_TPW) * HKV), block(256);
  float* lse = part + (size_t)B * HKV * ntile * (SKP_MAXQB * 32) * 2;
  const bool two = w * G > 128;  // query blocks per wave
#define SNAP_PASS(G_, NJQ_, P2_)                                                                                      \
  {                                                                                                                   \
    auto kern = snapkv_paged_kernel<T, D, G_, NJQ_, P2_, F8>;                                                         \
    set_dyn_lds_once(kern, (int)SKP_SMEM);                                                                            \
    hipLaunchKernelGGL(kern, grid, block, SKP_SMEM, st, (const uint16_t*)q, (const uint16_t*)k, sq_n, sk_n, sk_h,     \
                       (const uint8_t*)kc, ksc, page_table, bmap, scores, part, (const float*)lse, cu_q, cu_new, cu_k, \
                       B, HKV, w, w_b, ntile, c, pool, pool_tile, PS, NLP);                                           \
  }
#define SNAP2(G_, NJQ_)                                                                                               \
  {                                                                                                                   \
    SNAP_PASS(G_, NJQ_, false)                                                                                        \
    launch_snapkv_lse(part, lse, cu_k, B, HKV, w, w_b, G_, ntile, st);                                                \
    SNAP_PASS(G_, NJQ_, true)                                                                                         \
  }
#define SNAP(G_)                                                                                                      \
  {                                                                                                                   \
    if (two) SNAP2(G_, 2) else SNAP2(G_, 1)                                                                           \
  }
  switch (G) {
    case 1: SNAP(1); break;
    case 2: SNAP(2); break;
    case 4: SNAP(4); break;
    case 8: SNAP(8); break;
    default: return CVLLM_ERR_SHAPE;
  }
#undef SNAP_PASS
#undef SNAP2
#undef SNAP
  return check_launch();
}

}  // namespace cvllm

using namespace cvllm;

extern "C" int cvllm_snapkv_scores_paged(const void* q, const void* k, int64_t sq_n, int64_t sk_n, int64_t sk_h,
                                         const void* k_cache, const float* k_scale, const int32_t* page_table,
                                         const int32_t* batch_mapping, float* scores, const int32_t* cu_seqlens_q,
                                         const int32_t* cu_seqlens_new, const int32_t* cu_seqlens_k,
                                         const int32_t* window_b, int B, int HQ, int HKV, int D, int w, float sm_scale,
                                         int pool, int pool_tile, int max_seqlen_k, int page_size,
                                         int n_logical_pages_max, int cache_fp8, int dtype, void* workspace,
                                         size_t workspace_bytes, cvllm_stream_t stream) {
  if (!q || !k || !k_cache || !page_table || !batch_mapping || !scores || !cu_seqlens_q || !cu_seqlens_new ||
      !cu_seqlens_k)
    return CVLLM_ERR_ARG;
  if (cache_fp8 != 0 && cache_fp8 != 1) return CVLLM_ERR_ARG;
  if (cache_fp8 && !k_scale) return CVLLM_ERR_ARG;
  if (B <= 0 || HQ <= 0 || HKV <= 0 || max_seqlen_k <= 0 || pool <= 0 || page_size <= 0 || n_logical_pages_max <= 0)
    return CVLLM_ERR_ARG;
  if (pool_tile == 0) pool_tile = SKP_TILE;
  if (pool_tile != 32 && pool_tile != 64 && pool_tile != 128) return CVLLM_ERR_SHAPE;
  if (HQ % HKV != 0) return CVLLM_ERR_SHAPE;
  const int G = HQ / HKV;
  if (G != 1 && G != 2 && G != 4 && G != 8) return CVLLM_ERR_SHAPE;
  if (w <= 0 || w * G > SKP_MAXQB * 32) return CVLLM_ERR_SHAPE;
  if (D != 64 && D != 128) return CVLLM_ERR_SHAPE;
  if (dtype != CVLLM_F16 && dtype != CVLLM_BF16) return CVLLM_ERR_SHAPE;
  if ((sq_n % 8) || (sk_n % 8) || (sk_h % 8)) return CVLLM_ERR_SHAPE;
  if (!workspace || workspace_bytes < cvllm_snapkv_workspace_bytes(B, HKV, w, max_seqlen_k)) return CVLLM_ERR_WORKSPACE;
  const int ntile = (max_seqlen_k + SKP_TILE - 1) / SKP_TILE;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
#define SNAPD(T_, D_)                                                                                                  \
  return cache_fp8 ? snapkv_paged_g<T_, D_, true>(G, q, k, sq_n, sk_n, sk_h, k_cache, k_scale, page_table,             \
                                                  batch_mapping, scores, part, cu_seqlens_q, cu_seqlens_new,           \
                                                  cu_seqlens_k, B, HKV, w, window_b, ntile, sm_scale, pool, pool_tile, \
                                                  page_size, n_logical_pages_max, st)                                  \
                   : snapkv_paged_g<T_, D_, false>(G, q, k, sq_n, sk_n, sk_h, k_cache, k_scale, page_table,            \
                                                   batch_mapping, scores, part, cu_seqlens_q, cu_seqlens_new,          \
                                                   cu_seqlens_k, B, HKV, w, window_b, ntile, sm_scale, pool,           \
                                                   pool_tile, page_size, n_logical_pages_max, st)
  if (dtype == CVLLM_F16 && D == 128) SNAPD(F16, 128);
  if (dtype == CVLLM_F16 && D == 64) SNAPD(F16, 64);
  if (dtype == CVLLM_BF16 && D == 128) SNAPD(BF16, 128);
  SNAPD(BF16, 64);
#undef SNAPD
}
