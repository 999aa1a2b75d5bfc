"""GPU: prefill attention over an MXFP4 cached prefix (`cvllm_prefill_attn_mxfp4`), in-place compaction of an MXFP4 cache,
and what they switch on with `LLMConfig.mxfp4_prefix_reads`: chunked prefill and prefix reuse on an MXFP4 cache."""
import math

import pytest
import torch

import test_gpu_chunked_prefill as chunked
from helpers import mk_paged, tol
from oracle import ref_cpu as O
from test_gpu_kv_mxfp4 import code_values, dequantize, quantize_rows
from tiny_model import TinyConfig, TinyModel

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]


def _attend(dev, dtype, B, HQ, HKV, D, PS, lens, append, q_every7=1.0, k_mul=1.0, launches=1):
    """One problem: MXFP4 prefix of `lens` rows per head (shuffled pages, batch_mapping != arange; every code and scale
    byte the page table does not name within a length is 0xFF - a NaN scale), appended k / v as strided views of one fused
    buffer.  Returns the kernel's outputs and `O.prefill_attention` over the dequantised caches in float64."""
    from compactor_vllm_amd.attention.sparse_varlen_kernel import causal_sparse_varlen_with_cache

    g = torch.Generator().manual_seed(B * 1000 + D + PS + sum(append))
    kf, vf, pt, bm, _ = mk_paged(B, HKV, D, PS, lens, torch.float32, seed=7)
    (kq, ks), (vq, vs) = quantize_rows(kf), quantize_rows(vf)
    kd, vd = dequantize(kq, ks), dequantize(vq, vs)  # before the fill: the reference reads named rows only
    named = torch.zeros(kf.shape[0], dtype=torch.bool)
    for b in range(B):
        for h in range(HKV):
            named[O.cache_rows(pt[int(bm[b]), h], int(lens[b, h]), PS)] = True
    for t in (kq, ks, vq, vs):
        t[~named] = 0xFF
    N = sum(append)
    cu = torch.tensor([0] + append, dtype=torch.int32).cumsum(0).to(torch.int32)
    q = torch.randn(N, HQ, D, generator=g)
    q[::7] *= q_every7
    kv = torch.randn(N, 2 * HKV, D, generator=g)
    kv[:, :HKV] *= k_mul
    q, kv = q.to(dtype), kv.to(dtype)
    scale = 1.0 / math.sqrt(D)
    dv = [t.to(dev) for t in (q, kv, kq, vq, lens, pt, bm, cu, ks, vs)]
    outs = [causal_sparse_varlen_with_cache(dv[0], dv[1][:, :HKV], dv[1][:, HKV:], dv[2], dv[3], dv[4], dv[5], dv[6], dv[7],
                                            max(append), int(lens.max()), HKV, PS, scale, k_scale=dv[8], v_scale=dv[9])
            for _ in range(launches)]
    torch.cuda.synchronize()
    ref = O.prefill_attention(q, kv[:, :HKV], kv[:, HKV:], kd, vd, lens, pt, bm, cu, HKV, PS, scale)
    return [o.cpu() for o in outs], ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,HQ,HKV,D,PS,cache_max,append", [
    (2, 16, 2, 128, 128, 200, [130, 70]),     # G = 8
    (3, 8, 8, 128, 128, 140, [64, 65, 2]),    # G = 1
    (2, 16, 2, 64, 32, 150, [70, 200]),       # D = 64 (operand-split staging), a tile spans pages
    (2, 16, 4, 128, 96, 300, [130, 257]),     # tiles straddle page boundaries: the per-row page path
    (1, 4, 4, 128, 256, 513, [300]),          # prefix longer than the block; last cached tile is 1 row
    (2, 32, 8, 128, 64, 700, [1, 300]),       # append of 1 row; many pages on the scalar walk
])
def test_prefill_mxfp4_against_float64(dev, dtype, B, HQ, HKV, D, PS, cache_max, append):
    g = torch.Generator().manual_seed(cache_max)
    lens = torch.randint(1, cache_max + 1, (B, HKV), generator=g, dtype=torch.int32)
    lens[0, 0], lens[-1, -1] = 0, cache_max
    (out,), ref = _attend(dev, dtype, B, HQ, HKV, D, PS, lens, append)
    err = float((out.double() - ref.double()).abs().max())
    print(f"mxfp4 prefill {dtype} B{B} HQ{HQ} HKV{HKV} D{D} PS{PS} Lc{cache_max} La{append}: max abs err {err:.3e}")
    assert torch.isfinite(out.float()).all() and torch.allclose(out.double(), ref.double(), rtol=1e-6, atol=tol(dtype)), err


@pytest.mark.parametrize("dtype", DTYPES)
def test_prefill_mxfp4_large_logit_jump_across_the_seam(dev, dtype):
    """Appended keys x 4, every 7th query x 6: the row max jumps where the MXFP4 tiles end and the 16-bit tiles begin."""
    lens = torch.full((1, 2), 100, dtype=torch.int32)
    (o1, o2), ref = _attend(dev, dtype, 1, 8, 2, 128, 128, lens, [200], q_every7=6.0, k_mul=4.0, launches=2)
    assert torch.equal(o1, o2) and torch.isfinite(o1.float()).all()
    assert torch.allclose(o1.double(), ref.double(), rtol=1e-6, atol=tol(dtype)), (o1.double() - ref.double()).abs().max()


@pytest.mark.parametrize("D", [64, 128])
def test_compact_inplace_mxfp4_is_bit_exact(dev, D):
    """store_all + select + in-place compaction == compaction from the packed 16-bit rows into a fresh MXFP4 cache, code
    values and scale bytes at the kept slots; rows outside the sequences' original extents keep their fill pattern."""
    from compactor_vllm_amd.compression.common import compact_cache_inplace, extract_and_store_top_kv, select_retained
    from compactor_vllm_amd.kv_cache.store_kv_cache import prefill_store_all_kv

    B, HKV, PS, seqlens, N, P = 2, 2, 32, [300, 70], 370, 10
    g = torch.Generator().manual_seed(D)
    k, v = (torch.randn(N, HKV, D, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    sc = torch.randn(N, HKV, generator=g).to(dev)
    pt = torch.randperm((B + 1) * HKV * P, generator=g).view(B + 1, HKV, P).to(torch.int32)
    rows = ((B + 1) * HKV * P + 2) * PS
    bm = torch.tensor([2, 1], dtype=torch.int32)
    cu = torch.tensor([0, 300, 370], dtype=torch.int32, device=dev)
    retain = torch.tensor([300 * HKV // 2, 70 * HKV // 2], dtype=torch.int32, device=dev)
    zero = torch.zeros(B, HKV, dtype=torch.int32, device=dev)
    ptd, bmd = pt.to(dev), bm.to(dev)

    def fresh():
        return [torch.full((rows, w), fill, dtype=torch.uint8, device=dev)
                for w, fill in ((D // 2, 0x55), (D // 2, 0x55), (D // 32, 0xA7), (D // 32, 0xA7))]

    want, got = fresh(), fresh()
    _, lens_w = extract_and_store_top_kv(sc, cu, 300, 300 * HKV, HKV, k, v, retain, ptd, bmd, zero.clone(), want[0], want[1],
                                         PS, k_scale=want[2], v_scale=want[3])
    prefill_store_all_kv(new_keys=k, new_values=v, cu_seqlens_k=cu, max_seqlen_k=300, k_cache=got[0], v_cache=got[1],
                         page_table=ptd, bh_lens=zero.clone(), batch_mapping=bmd, PAGE_SIZE=PS, k_scale=got[2], v_scale=got[3])
    kept, lens_g = select_retained(sc, cu, 300, retain, bmd, zero, PS, True)
    compact_cache_inplace(kept, lens_g, zero, zero, ptd, bmd, got[0], got[1], PS, k_scale=got[2], v_scale=got[3])
    torch.cuda.synchronize()
    assert torch.equal(lens_g, lens_w)
    want, got = [t.cpu() for t in want], [t.cpu() for t in got]
    outside = torch.ones(rows, dtype=torch.bool)
    for b in range(B):
        for h in range(HKV):
            r = O.cache_rows(pt[int(bm[b]), h], int(lens_g[b, h]), PS)
            for i, (a, w) in enumerate(zip(got, want)):
                assert torch.equal(code_values(a[r]), code_values(w[r])) if i < 2 else torch.equal(a[r], w[r]), (b, h, i)
            outside[O.cache_rows(pt[int(bm[b]), h], seqlens[b], PS)] = False
    assert all((t[outside] == fill).all() for t, fill in zip(got, (0x55, 0x55, 0xA7, 0xA7)))


def test_one_layer_chunked_on_mxfp4_cache(dev, monkeypatch):
    """The `Attention` module fed 1536 tokens in chunks of 512 on an MXFP4 cache, COMPACTOR at 0.5: every chunk's output is
    attention over [dequantised earlier rows || the chunk]; afterwards the cache holds `quantize_rows` of the kept tokens."""
    from compactor_vllm_amd.compression import CompressionMethod

    plain_layer = chunked._layer

    def mxfp4_layer(dev_, HQ, HKV, D, PS, total, dtype):
        cache, attn, row = plain_layer(dev_, HQ, HKV, D, PS, total, torch.uint8)
        attn.k_scale, attn.v_scale = cache.layer_scale_slices(0)
        return cache, attn, row

    monkeypatch.setattr(chunked, "_layer", mxfp4_layer)
    dtype, HQ, HKV, D, PS, first, last, total, cuts = torch.bfloat16, 8, 2, 128, 128, 4, 8, 1536, [0, 512, 1024, 1536]
    g = torch.Generator().manual_seed(1536)
    mk = lambda h, s=0.5: (torch.randn(total, h, D, generator=g) * s).to(dtype).to(dev)  # noqa: E731
    q_pre, k_pre, q, k, v = mk(HQ), mk(HKV), mk(HQ), mk(HKV), mk(HKV, 1.0)
    PHI = (torch.randn(D, 48, generator=g) / math.sqrt(48)).to(dtype).to(dev)
    retain = torch.tensor([O.retain_count(0.5, total, first, last, HKV)], dtype=torch.int32, device=dev)
    out, sc, attn, row, _ = chunked._run(dev, CompressionMethod.COMPACTOR, q_pre, k_pre, q, k, v, cuts, retain, PHI,
                                         first, last, HQ, HKV, D, PS, dtype)
    qc, kc, vc = q.cpu(), k.cpu(), v.cpu()
    (kq, ks), (vq, vs) = quantize_rows(kc), quantize_rows(vc)  # [total, HKV, D/2], [total, HKV, D/32]
    P = total // PS
    deq = [dequantize(c, s).transpose(0, 1).reshape(HKV * P * PS, D) for c, s in ((kq, ks), (vq, vs))]
    pt0, bm0 = torch.arange(HKV * P, dtype=torch.int32).view(1, HKV, P), torch.zeros(1, dtype=torch.int32)
    for s0, s1 in zip(cuts[:-1], cuts[1:]):
        ref = O.prefill_attention(qc[s0:s1], kc[s0:s1], vc[s0:s1], deq[0], deq[1], torch.full((1, HKV), s0), pt0, bm0,
                                  torch.tensor([0, s1 - s0]), HKV, PS, 1.0 / math.sqrt(D))
        assert torch.allclose(out[s0:s1].cpu().double(), ref.double(), rtol=1e-6, atol=tol(dtype)), s0
    kept, lens_o = O.retained_sets(sc.cpu(), torch.tensor([0, total], dtype=torch.int32), retain.cpu(),
                                   torch.zeros(1, HKV, dtype=torch.int32), torch.tensor([row], dtype=torch.int32), PS, True)
    assert torch.equal(attn.bh_seq_lens[row].cpu()[None], lens_o)
    for h in range(HKV):
        r, src = O.cache_rows(attn.page_table[row, h].cpu(), int(lens_o[0, h]), PS), sorted(kept[0][h])
        for cache, codes, scale_arr, scales in ((attn.k_cache, kq, attn.k_scale, ks), (attn.v_cache, vq, attn.v_scale, vs)):
            assert torch.equal(code_values(cache.cpu()[r]), code_values(codes[src, h])), h
            assert torch.equal(scale_arr.cpu()[r], scales[src, h]), h


def _llm(dev):
    from compactor_vllm_amd import LLM, LLMConfig

    cfg = TinyConfig()
    conf = LLMConfig(model="tiny", max_num_seqs=4, max_model_len=4096, hf_config=cfg, kvcache_page_size=128,
                     enforce_eager=True, show_progress_bar=False, kv_cache_dtype="mxfp4", mxfp4_prefix_reads=True)
    return LLM(conf, TinyModel(cfg, dev), device=dev, num_pages=200, max_batched_tokens=1024)


def test_engine_chunked_prefill_on_mxfp4_cache(dev):
    """A 3 000-token prompt (three chunks) next to two short ones: every request equals its run alone, token for token;
    nothing leaks; SnapKV, whose scoring cannot read 4-bit rows, refuses the chunked prompt."""
    from compactor_vllm_amd import BatchCompressionParams, CompressionMethod, SamplingParams, SequenceCompressionParams

    g = torch.Generator().manual_seed(4)
    prompts = [torch.randint(0, 512, (n,), generator=g).tolist() for n in (3000, 200, 640)]
    sp = SamplingParams(temperature=0.0, max_new_tokens=6)
    scp = lambda: SequenceCompressionParams(0.5, 4, 16)  # noqa: E731
    llm = _llm(dev)
    mgr = llm.master_model_runner.kv_manager
    assert mgr.chunked_prefill and mgr.mxfp4_prefix_reads and mgr.paged_cache.kv_cache.dtype == torch.uint8
    out = llm.generate(prompts, sp, per_sequence_compression_params=[scp() for _ in prompts])
    assert mgr.num_free_pages == 200 and mgr.num_free_batches == 4
    solo = _llm(dev)
    for i, p in enumerate(prompts):
        assert solo.generate([p], sp, per_sequence_compression_params=scp())[0] == out[i] and len(out[i]) == 7, i
    with pytest.raises(NotImplementedError, match="SnapKV"):
        solo.generate([prompts[0]], sp, BatchCompressionParams(compression_method=CompressionMethod.SNAPKV),
                      per_sequence_compression_params=scp())


@pytest.mark.parametrize("method_name,ratio", [("COMPACTOR", 0.5), ("NONE", 1.0)])
def test_prefix_reuse_on_mxfp4_cache(dev, method_name, ratio):
    """cache_prefix of 1 024 tokens, then a 1 600-token request == a cold chunked prefill whose first cut falls at 1 024."""
    from compactor_vllm_amd import BatchCompressionParams, CompressionMethod, SamplingParams, SequenceCompressionParams

    bcp = BatchCompressionParams(compression_method=CompressionMethod[method_name])
    scp = lambda: SequenceCompressionParams(ratio, protected_first_tokens=4, protected_last_tokens=16)  # noqa: E731
    sp = SamplingParams(temperature=0.0, max_new_tokens=6)
    prompt = torch.randint(0, 512, (1600,), generator=torch.Generator().manual_seed(23)).tolist()
    cold = _llm(dev).generate([prompt], sp, bcp, per_sequence_compression_params=scp())
    warm = _llm(dev)
    assert warm.cache_prefix(prompt[:1024], bcp) == 1024
    out = warm.generate([prompt], sp, bcp, per_sequence_compression_params=scp())
    assert next(iter(warm.master_model_runner.prefix_cache.entries.values())).hits == 1
    assert out[0] == cold[0]
