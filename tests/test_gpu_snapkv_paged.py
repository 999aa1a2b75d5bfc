"""GPU: SnapKV scores with the keys read in place, [paged cache prefix (16 bit / FP8) || packed chunk]
(cvllm_snapkv_scores_paged), against the plain kernel on the gathered keys (bit for bit) and the CPU oracle."""
import math

import pytest
import torch

from helpers import mk_paged
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

W = 32
SHAPES = [  # HQ, HKV, D, PS, prefix P_b, new tokens, pool_tile
    (8, 2, 128, 128, [512, 0], [300, 161], 128),  # aligned whole-page tiles; a sequence without a prefix; B = 2
    (16, 2, 128, 32, [77], [100], 128),           # G = 8; seam inside a tile and a page; a tile spanning four pages
    (4, 4, 64, 32, [645], [40], 128),             # D = 64, G = 1; seam in the second group; L - w close behind it
    (8, 2, 128, 128, [1100], [436], 128),         # three groups; seam mid-page at PS 128; last tile partial
    (16, 2, 128, 32, [77], [100], 32),
]


@pytest.mark.parametrize("cache,dtype", [("16", torch.bfloat16), ("16", torch.float16), ("fp8", torch.bfloat16),
                                         ("fp8", torch.float16)])
@pytest.mark.parametrize("HQ,HKV,D,PS,prefix,new,pool_tile", SHAPES)
def test_paged_scores_equal_gathered_and_oracle(dev, cache, dtype, HQ, HKV, D, PS, prefix, new, pool_tile):
    from compactor_vllm_amd import _lib
    from compactor_vllm_amd.compression.snapkv import query_aware_key_scores, query_aware_key_scores_paged

    B = len(prefix)
    g = torch.Generator().manual_seed(HQ + D + PS + sum(prefix))
    lens_bh = torch.tensor(prefix)[:, None].expand(B, HKV)
    k_cache, _, pt, bm, _ = mk_paged(B, HKV, D, PS, lens_bh, dtype, seed=sum(new))
    live = torch.zeros(k_cache.shape[0], dtype=torch.bool)
    rows = [[O.cache_rows(pt[int(bm[b]), h], prefix[b], PS) for h in range(HKV)] for b in range(B)]
    for b in range(B):
        for h in range(HKV):
            live[rows[b][h]] = True
    # cache rows at or past P_b are poison: the kernel may not read them
    if cache == "fp8":
        scale = (k_cache.float().abs().amax(dim=1) / 448.0).clamp_min(1e-6)
        codes = (k_cache.float() / scale[:, None]).to(_lib.FP8)
        codes.view(torch.uint8)[~live] = 0x7F
        scale[~live] = float("nan")
        readback = lambda r: (codes.view(torch.uint8)[r].view(_lib.FP8).float() * scale[r][:, None]).to(dtype)  # noqa: E731
        kc_dev, ks_dev = codes.to(dev), scale.to(dev)
    else:
        k_cache[~live] = float("nan")
        readback = lambda r: k_cache[r]  # noqa: E731
        kc_dev, ks_dev = k_cache.to(dev), None
    N_new = sum(new)
    wide = (torch.randn(N_new, HKV + 1, D + 8, generator=g) * 0.5).to(dtype).to(dev)
    k = wide[:, 1:, 8:]  # a strided view: row and head strides are not the packed ones
    q = (torch.randn(N_new, HQ, D, generator=g) * 0.5).to(dtype).to(dev)
    cu = lambda xs: torch.tensor([0] + list(torch.tensor(xs).cumsum(0)), dtype=torch.int32)  # noqa: E731
    cu_new, cu_k = cu(new), cu([p + n for p, n in zip(prefix, new)])
    # what the hook used to build: every sequence's [read-back prefix || new keys]
    k_all = torch.cat([torch.cat([torch.stack([readback(rows[b][h]) for h in range(HKV)], 1),
                                  k[cu_new[b]:cu_new[b + 1]].cpu()]) for b in range(B)])
    got = query_aware_key_scores_paged(q, k, cu_new.to(dev), cu_new.to(dev), cu_k.to(dev), kc_dev, pt.to(dev),
                                       bm.to(dev), PS, W, k_scale=ks_dev, max_seqlen_k=int(cu_k.diff().max()),
                                       pool_tile=pool_tile)
    plain = query_aware_key_scores(q, k_all.to(dev), cu_new.to(dev), cu_k.to(dev), W, pool_tile=pool_tile)
    torch.cuda.synchronize()
    assert got.shape == plain.shape and torch.equal(got, plain)                      # (a)
    ref = O.snapkv_scores(q.cpu(), k_all, cu_new, cu_k, W, pool_tile=pool_tile)
    got = got.cpu()
    assert not torch.isnan(got).any()                                                # (c)
    fin = torch.isfinite(ref)
    assert torch.equal(fin, torch.isfinite(got))                                     # (b)
    assert torch.allclose(got[fin], ref[fin], rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("cache_dtype", [torch.bfloat16, torch.float8_e4m3fn])
def test_chunked_hook_uses_paged_kernel_without_key_copy(dev, cache_dtype):
    """One layer, 1536 tokens in chunks of 512: the last chunk's SnapKV scoring allocates less than ONE [total, HKV, D]
    16-bit tensor (scores + workspace are (2 ntile + 1) KiB per head; a copy of the keys is ntile * 32 KiB per head)."""
    from compactor_vllm_amd.compression import CompressionMethod, apply_postrope_compression
    from compactor_vllm_amd.kv_cache.page_table import PagedKVCache
    from compactor_vllm_amd.layers.attention import Attention
    from compactor_vllm_amd.utils.chunked import ChunkedPrefillState, PrefillChunk
    from compactor_vllm_amd.utils.context import CompressionContext, get_context, set_context

    dtype, HQ, HKV, D, PS, total, chunk = torch.bfloat16, 8, 2, 128, 128, 1536, 512
    npg = total // PS + 1
    cache = PagedKVCache(num_layers=1, max_logical_pages_per_head=npg, num_pages=HKV * npg * 3, page_size=PS, H_kv=HKV,
                         head_dim=D, max_num_batches=3, dtype=cache_dtype, device=dev)
    cache.new_batch()
    row = cache.new_batch()
    assert cache.reserve_tokens(row, total + 4).name == "SUCCESS"
    attn = Attention(HQ, D, 1.0 / math.sqrt(D), HKV)
    attn.k_cache, attn.v_cache, attn.page_table, attn.bh_seq_lens = cache.layer_slices(0)
    if cache_dtype == torch.float8_e4m3fn:
        attn.k_scale, attn.v_scale = cache.layer_scale_slices(0)
    attn.page_size = PS
    g = torch.Generator().manual_seed(5)
    mk = lambda h: (torch.randn(total, h, D, generator=g) * 0.5).to(dtype).to(dev)  # noqa: E731
    q, k, v = mk(HQ), mk(HKV), mk(HKV)
    bm = torch.tensor([row], dtype=torch.int32, device=dev)
    retain = torch.tensor([O.retain_count(0.25, total, 4, 8, HKV)], dtype=torch.int32, device=dev)
    state = ChunkedPrefillState(total, HKV, [attn])
    store = torch.cuda.Stream()
    rise = None
    for s0 in range(0, total, chunk):
        last = s0 + chunk == total
        cu = torch.tensor([0, chunk], dtype=torch.int32, device=dev)
        cc = CompressionContext(compression_method=CompressionMethod.SNAPKV, compression_chunk_size=-1,
                                batch_tokens_to_retain=retain, max_tokens_to_retain=total * HKV,
                                context_lens=[chunk], PHI=None, protected_first_tokens=[4], protected_last_tokens=[8])
        state.begin_chunk()
        set_context(is_prefill=True, do_compression=True, cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=chunk,
                    max_seqlen_k=chunk, batch_mapping=bm, max_bh_len=s0, compression_context=cc, STORE_STREAM=store,
                    chunk=PrefillChunk(s0, chunk, last, state))
        sl = slice(s0, s0 + chunk)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        sc = apply_postrope_compression(q[sl], k[sl], v[sl], None, get_context())
        torch.cuda.current_stream().wait_stream(store)
        torch.cuda.synchronize()
        if last:
            rise = torch.cuda.max_memory_allocated() - base
        attn(q[sl], k[sl], v[sl], sc)
        torch.cuda.current_stream().wait_stream(store)
        torch.cuda.synchronize()
    assert sc is not None and sc.shape == (total, HKV)
    assert rise < total * HKV * D * 2, rise
