"""Causal varlen prefill attention over [paged KV prefix || appended block] (MI355X MFMA kernel).

Mirror of the reference module `compactor_vllm/attention/sparse_varlen_kernel.py`
(wrapper :11-197): same name, argument order and assertions; the Triton kernel (:277-519) is
replaced by `cvllm_prefill_attn` (`cvllm_prefill_attn_fp8` over an FP8 cache, `cvllm_prefill_attn_mxfp4` over an MXFP4
cache with a non-empty prefix).
"""
from __future__ import annotations

import math

import torch

from .. import _lib


def causal_sparse_varlen_with_cache(
    q,
    k,
    v,
    k_cache,
    v_cache,
    seq_lens_bh,
    global_page_table,
    batch_mapping,
    cu_seqlens_q,
    max_seqlen_q: int,
    max_seqlen_k_cache: int,
    HKV: int,
    PAGE_SIZE: int,
    sm_scale=None,
    k_scale=None,
    v_scale=None,
):
    """out = softmax_causal(q [K_prefix || k]^T * scale) [V_prefix || v] per sequence and kv-head.

    q [N, HQ, D]; k, v [N, HKV, D] (last dim contiguous, arbitrary token stride — the model passes
    strided views of the fused qkv buffer); k_cache / v_cache [CACHE_SIZE, D]; seq_lens_bh [B, HKV] =
    cached prefix lengths BEFORE this step (per kv-head); global_page_table [MAX_BATCHES, HKV, P];
    batch_mapping [B]; cu_seqlens_q [B+1].  With an FP8 cache (k_cache.dtype float8_e4m3fn: e4m3 codes) `k_scale` /
    `v_scale` [CACHE_SIZE] fp32 are the rows' scales and the kernel is `cvllm_prefill_attn_fp8`: a cached element is read
    back as (fp32(code) * scale) rounded to q.dtype.  With an MXFP4 cache (uint8: [CACHE_SIZE, D/2] e2m1 codes) they
    are [CACHE_SIZE, D/32] uint8 block scales and a cached element is read back as fp32(code) * 2^E
    (`cvllm_prefill_attn_mxfp4`).  `max_seqlen_k_cache` only keys the reference's autotuner (quirk Q10) and is ignored -
    except on an MXFP4 cache, where 0 (what the engine passes for a prefill that is neither a chunk nor a prefix hit)
    means "no prefix": the 16-bit kernel then runs on zeroed lengths and the cache is never dereferenced.  Returns
    [N, HQ, D] contiguous in q.dtype.
    """
    assert q.ndim == 3, "q should be [N, HQ, D]"
    N, HQ, D = q.shape
    assert (D & (D - 1)) == 0, "D must be power of two"
    B = cu_seqlens_q.numel() - 1
    assert B > 0
    assert HQ % HKV == 0, "Number of query heads must divide number of keys heads"
    assert k.shape == (N, HKV, D) and v.shape == (N, HKV, D)
    assert q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1, "final dimension must be contiguous"
    assert q.stride(1) == D, "query heads must be contiguous"
    CACHE_SIZE = k_cache.shape[0]
    assert v_cache.shape[0] == CACHE_SIZE
    mxfp4 = k_cache.dtype == _lib.MXFP4
    mxfp4_prefix = mxfp4 and int(max_seqlen_k_cache) > 0
    if mxfp4:
        assert k_cache.shape[1] == D // 2 and v_cache.shape[1] == D // 2
        if not mxfp4_prefix:
            # No prefix anywhere in the batch (a plain prefill): the faster 16-bit kernel runs on zero prefix lengths (a
            # local array: it must never dereference the 4-bit cache).
            seq_lens_bh = torch.zeros_like(seq_lens_bh)
    else:
        assert k_cache.shape[1] == D and v_cache.shape[1] == D
    assert PAGE_SIZE > 0 and CACHE_SIZE % PAGE_SIZE == 0
    assert k_cache.is_contiguous() and v_cache.is_contiguous() and global_page_table.is_contiguous()
    _lib.require_cuda(q, k, v, k_cache, v_cache, seq_lens_bh, global_page_table, batch_mapping, cu_seqlens_q)
    if sm_scale is None:
        sm_scale = 1.0 / math.sqrt(D)

    cu = _lib.i32(cu_seqlens_q)
    lens = _lib.i32(seq_lens_bh)
    bm = _lib.i32(batch_mapping)
    pt = _lib.i32(global_page_table)
    out = torch.empty((N, HQ, D), dtype=q.dtype, device=q.device)
    args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
            k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(), lens.data_ptr(), pt.data_ptr(), bm.data_ptr(),
            cu.data_ptr(), B, N, int(max_seqlen_q), HQ, HKV, D, int(PAGE_SIZE), pt.shape[-1], float(sm_scale),
            _lib.dtype_code(q.dtype), _lib.stream())
    if k_cache.dtype == _lib.FP8:
        assert v_cache.dtype == _lib.FP8
        _lib.check_fp8_scales(k_cache, k_scale, v_scale)
        st = _lib.lib().cvllm_prefill_attn_fp8(*args, k_scale.data_ptr(), v_scale.data_ptr())
        _lib.check(st, "cvllm_prefill_attn_fp8")
    elif mxfp4_prefix:
        assert v_cache.dtype == _lib.MXFP4
        _lib.check_mxfp4_scales(k_cache, k_scale, v_scale)
        st = _lib.lib().cvllm_prefill_attn_mxfp4(*args, k_scale.data_ptr(), v_scale.data_ptr())
        _lib.check(st, "cvllm_prefill_attn_mxfp4")
    else:
        st = _lib.lib().cvllm_prefill_attn(*args)
        _lib.check(st, "cvllm_prefill_attn")
    return out
