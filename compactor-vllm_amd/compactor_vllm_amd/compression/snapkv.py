"""SnapKV query-aware key scoring on MI355X HIP kernels.

Mirror of the reference module `compactor_vllm/compression/snapkv.py`: `SnapKVCompression` (:12-36)
and `query_aware_key_scores` (:332-448) keep their names, argument order and defaults.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from .. import _lib
from ..utils.helpers import maybe_execute_in_stream
from .common import BaseCompressionMethod
from .compactor import zscore_segments_


class SnapKVCompression(BaseCompressionMethod):
    @staticmethod
    def pre_rope_scoring(q, k, v, context) -> Optional[torch.Tensor]:
        return None

    @staticmethod
    def post_rope_scoring(q, k, v, pre_rope_scores, context) -> Optional[torch.Tensor]:
        if getattr(context, "chunk", None) is not None:
            return maybe_execute_in_stream(_chunked_post_rope, q, k, context, STORE_STREAM=context.STORE_STREAM)
        return maybe_execute_in_stream(
            query_aware_key_scores,
            q,
            k,
            context.cu_seqlens_q,
            context.cu_seqlens_k,
            w=32,
            max_seqlen_k=context.max_seqlen_k,
            STORE_STREAM=context.STORE_STREAM,
        )


def _chunked_post_rope(q, k, context):
    """Chunked prefill (utils/chunked.py): SnapKV scores once, on the last chunk - the window's queries are in this
    chunk, the keys are [rows of the earlier chunks read back from this layer's cache || this chunk's keys]."""
    ch = context.chunk
    li = ch.state.next_layer()
    if not ch.is_last:
        return None
    attn = ch.state.attn[li]
    cu_k = torch.tensor([0, ch.total_len], dtype=torch.int32).to(k.device, non_blocking=True)
    return query_aware_key_scores_paged(
        q, k, context.cu_seqlens_q, context.cu_seqlens_k, cu_k, attn.k_cache, attn.page_table, context.batch_mapping,
        attn.page_size, w=32, k_scale=attn.k_scale, max_seqlen_k=ch.total_len)


def query_aware_key_scores_paged(
    q: torch.Tensor,  # [N_q, Hq, D]
    k: torch.Tensor,  # [N_new, Hk, D]: the keys that are not in the cache yet
    cu_seqlens_q: torch.Tensor,  # [B+1], int32
    cu_seqlens_new: torch.Tensor,  # [B+1], int32: rows of `k`
    cu_seqlens_k: torch.Tensor,  # [B+1], int32: all keys, cached prefix + new
    k_cache: torch.Tensor,  # [cache_rows, D], q.dtype or FP8 codes
    page_table: torch.Tensor,  # [Bmax, Hk, n_logical_pages] int32
    batch_mapping: torch.Tensor,  # [B] int32
    PAGE_SIZE: int,
    w: "torch.Tensor | int",
    sm_scale: float = None,
    *,
    k_scale: torch.Tensor = None,  # [cache_rows] fp32, with an FP8 cache
    max_seqlen_k: int = None,
    pool_tile: int = 128,
) -> torch.Tensor:
    """`query_aware_key_scores` with the keys read in place: sequence b's keys are its first
    P_b = L_b - L_new_b rows in the paged `k_cache` (per kv-head, through `page_table[batch_mapping[b]]`) followed by
    its rows of `k`.  An FP8 cache is read back as (fp32(code) * k_scale[row]) rounded to q.dtype, the prefill kernel's
    rule.  fp32 [sum L_b, Hk], bit-identical to `query_aware_key_scores` on the gathered keys; no copy of the keys is
    made.  No host sync when `max_seqlen_k` is given, `w` is an int and B = 1 (a batch's row count sum L_b is read
    from `cu_seqlens_k`)."""
    assert q.stride(-1) == 1 and k.stride(-1) == 1, "last dim must be contiguous"
    assert pool_tile in (32, 64, 128), "pool_tile must be one of the reference's BLOCK_K configurations"
    _lib.require_cuda(q, k, cu_seqlens_q, cu_seqlens_new, cu_seqlens_k, k_cache, page_table, batch_mapping)
    w_b = None
    if not isinstance(w, int):
        _lib.require_cuda(w)
        w_b = _lib.i32(w)
        assert w_b.numel() == cu_seqlens_q.numel() - 1
        w = int(w_b.max().item())
    N_q, Hq, D = q.shape
    N_new, Hk, Dk = k.shape
    assert (Hq % Hk) == 0, "Hq must be a multiple of Hk"
    assert q.stride(1) == D and k.dtype == q.dtype and Dk == D
    fp8 = k_cache.dtype == _lib.FP8
    assert k_cache.is_contiguous() and k_cache.shape[1] == D and (fp8 or k_cache.dtype == q.dtype)
    if fp8:
        _lib.check_fp8_scales(k_cache, k_scale, k_scale)
    assert page_table.dtype == torch.int32 and page_table.is_contiguous() and page_table.shape[1] == Hk
    if sm_scale is None:
        sm_scale = 1.0 / math.sqrt(D)
    B = cu_seqlens_q.numel() - 1
    assert B == cu_seqlens_k.numel() - 1 == cu_seqlens_new.numel() - 1 == batch_mapping.numel()
    cq, cn, ck = _lib.i32(cu_seqlens_q), _lib.i32(cu_seqlens_new), _lib.i32(cu_seqlens_k)
    bm = _lib.i32(batch_mapping)
    if max_seqlen_k is None:
        max_seqlen_k = int(ck.diff().max().item())
    # rows of the result, sum L_b: the one sequence's length (the engine's call), else read from cu_seqlens_k
    N_k = int(max_seqlen_k) if B == 1 else int(ck[-1].item())
    if w * (Hq // Hk) == 0:
        return torch.zeros((N_k, Hk), dtype=torch.float32, device=q.device)
    out = torch.empty((N_k, Hk), dtype=torch.float32, device=q.device)
    L = _lib.lib()
    ws_bytes = L.cvllm_snapkv_workspace_bytes(B, Hk, w, int(max_seqlen_k))
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=q.device)
    st = L.cvllm_snapkv_scores_paged(
        q.data_ptr(), k.data_ptr(), q.stride(0), k.stride(0), k.stride(1), k_cache.data_ptr(),
        _lib.ptr(k_scale) if fp8 else None, page_table.data_ptr(), bm.data_ptr(), out.data_ptr(),
        cq.data_ptr(), cn.data_ptr(), ck.data_ptr(), _lib.ptr(w_b), B, Hq, Hk, D, int(w), float(sm_scale), 5,
        int(pool_tile), int(max_seqlen_k), int(PAGE_SIZE), page_table.shape[2], int(fp8), _lib.dtype_code(q.dtype),
        ws.data_ptr(), ws_bytes, _lib.stream(),
    )
    _lib.check(st, "cvllm_snapkv_scores_paged")
    return out


def query_aware_key_scores(
    q: torch.Tensor,  # [N_q, Hq, D]
    k: torch.Tensor,  # [N_k, Hk, D]
    cu_seqlens_q: torch.Tensor,  # [B+1], int32
    cu_seqlens_k: torch.Tensor,  # [B+1], int32
    w: "torch.Tensor | int",  # [B] int32 or one window for every sequence
    sm_scale: float = None,  # defaults to 1/sqrt(D)
    *,
    accum_scores: torch.Tensor = None,
    accum_blending: float = None,
    normalize: bool = False,
    max_seqlen_k: int = None,
    pool_tile: int = 128,
) -> Optional[torch.Tensor]:
    """s_j = sum over the last `w` queries x G heads of softmax_row(q k^T / sqrt D) restricted to keys
    [0, L-w); trailing 5-tap mean clipped at the start of the key's `pool_tile`-wide block (counted from the sequence
    start): `pool_tile` in {32, 64, 128} is the BLOCK_K the reference's autotuner picked for its
    `_scores_from_logits_kernel` (snapkv.py:160-168, 253-262) - the pooled values depend on it, so a caller that must
    match a given reference box passes that box's outcome (default 128; extension argument);
    last w keys <- +inf.  fp32 [N_k, Hk].  `w` is an int (the engine passes 32) or a [B] int32 tensor of per-sequence
    windows (one host sync for its maximum, like the reference's `w.max().item()`).  normalize=True z-scores every
    sequence's scored rows [0, L-w) over all heads (biased variance, eps 1e-12 inside the square root; reference
    :279-329).  `max_seqlen_k` avoids a host sync; when omitted it is read from cu_seqlens_k.  Sequences with L <= w
    come back all +inf (reference: uninitialised)."""
    assert q.stride(-1) == 1 and k.stride(-1) == 1, "last dim must be contiguous"
    assert pool_tile in (32, 64, 128), "pool_tile must be one of the reference's BLOCK_K configurations"
    _lib.require_cuda(q, k, cu_seqlens_q, cu_seqlens_k)
    w_b = None
    if not isinstance(w, int):
        _lib.require_cuda(w)
        w_b = _lib.i32(w)
        assert w_b.numel() == cu_seqlens_q.numel() - 1
        w = int(w_b.max().item())
    N_q, Hq, D = q.shape
    N_k, Hk, Dk = k.shape
    assert (Hq % Hk) == 0, "Hq must be a multiple of Hk"
    assert q.stride(1) == D
    if sm_scale is None:
        sm_scale = 1.0 / math.sqrt(D)
    B = cu_seqlens_q.numel() - 1
    assert B == cu_seqlens_k.numel() - 1
    if w * (Hq // Hk) == 0:
        return torch.zeros((N_k, Hk), dtype=torch.float32, device=q.device)
    cq, ck = _lib.i32(cu_seqlens_q), _lib.i32(cu_seqlens_k)
    if max_seqlen_k is None:
        max_seqlen_k = int(ck.diff().max().item())
    out = torch.empty((N_k, Hk), dtype=torch.float32, device=q.device)
    L = _lib.lib()
    ws_bytes = L.cvllm_snapkv_workspace_bytes(B, Hk, w, int(max_seqlen_k))
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=q.device)
    st = L.cvllm_snapkv_scores_wb(
        q.data_ptr(), k.data_ptr(), q.stride(0), k.stride(0), k.stride(1), out.data_ptr(), cq.data_ptr(), ck.data_ptr(),
        _lib.ptr(w_b), B, Hq, Hk, D, int(w), float(sm_scale), 5, int(pool_tile), int(max_seqlen_k),
        _lib.dtype_code(q.dtype),
        ws.data_ptr(), ws_bytes, _lib.stream(),
    )
    _lib.check(st, "cvllm_snapkv_scores_wb")
    if normalize:
        zb = L.cvllm_zscore_workspace_bytes(B)
        zws = torch.empty(max(zb, 4), dtype=torch.uint8, device=q.device)
        st = L.cvllm_zscore_windowed(out.data_ptr(), 2, ck.data_ptr(), _lib.ptr(w_b), int(w), B, Hk, 1e-12, N_k,
                                     zws.data_ptr(), zb, _lib.stream())
        _lib.check(st, "cvllm_zscore_windowed")
    if accum_scores is not None:
        if accum_blending is not None:
            accum_scores.mul_(accum_blending)
        accum_scores.add_(out)
        return accum_scores
    return out
