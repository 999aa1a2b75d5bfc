"""GPU: the MXFP4 (OCP e2m1 codes + e8m0 block scales) paged KV cache - the quantising stores against a CPU restatement
of the format, decode attention over an MXFP4 cache against a float64 reference, and the engine with
`kv_cache_dtype="mxfp4"`."""
import math

import pytest
import torch

from helpers import mk_paged, tol
from oracle import ref_cpu as O
from tiny_model import TinyConfig, TinyModel

pytestmark = pytest.mark.gpu
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def quantize_rows(x):
    """The format restated in torch: x [..., D] -> (codes uint8 [..., D/2], scales uint8 [..., D/32])."""
    xf = x.float().reshape(*x.shape[:-1], -1, 32)
    a = xf.abs().amax(dim=-1)
    s = (((a.view(torch.int32) >> 23) & 0xFF) - 2).clamp_min(0)          # exponent field of the block maximum, minus 2
    y = torch.ldexp(xf.abs(), (127 - s)[..., None])                       # |x| * 2^-E, exact
    code = ((y > 0.25).int() + (y >= 0.75).int() + (y > 1.25).int() + (y >= 1.75).int() + (y > 2.5).int()
            + (y >= 3.5).int() + (y > 5.0).int())                         # the seven midpoints, ties to the even code
    code = (code | ((xf < 0).int() << 3)).reshape(*x.shape[:-1], -1, 2)
    return (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8), s.to(torch.uint8)


def code_values(codes):
    """[..., D/2] packed bytes -> [..., D] float64 e2m1 values (so that +0 and -0 compare equal)."""
    nib = torch.stack([codes & 15, codes >> 4], dim=-1).reshape(*codes.shape[:-1], -1).long()
    return E2M1[nib & 7] * (1 - 2 * (nib >> 3)).double()


def dequantize(codes, scales):
    v = code_values(codes)
    return (v.reshape(*scales.shape, 32) * torch.exp2(scales.double() - 127)[..., None]).reshape(v.shape)


@pytest.mark.parametrize("src_dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
def test_stores_follow_the_format(dev, D, src_dtype):
    """store_all, the compaction behind extract_and_store_top_kv and decode_store_kv write exactly the scale bytes and
    the code values of the restatement at the rows the page table names (rows cross page boundaries), nothing else."""
    from compactor_vllm_amd.compression.common import extract_and_store_top_kv
    from compactor_vllm_amd.config.constants import RESERVED_BATCH
    from compactor_vllm_amd.kv_cache.store_kv_cache import decode_store_kv, prefill_store_all_kv

    B, HKV, PS, P = 2, 2, 32, 4
    seqlens = [37, 70]
    N = sum(seqlens)
    g = torch.Generator().manual_seed(D + (src_dtype == torch.float16))
    kv = torch.randn(N, 2 * HKV, D, generator=g)
    kv[3, 0] = 0.0                       # all-zero row (K)
    kv[3, HKV + 1] = 0.0                 # (V)
    kv[40, 1, 7] = 1e4                   # an outlier in one block only
    kv[41, HKV, 40] = -1e4
    kv[50] *= 1e-3                       # small magnitude
    ties = torch.tensor([7.0, 0.75, 2.5, 5.0, -0.75, -2.5, -5.0, 0.25, 1.25, 1.75, 3.5, -7.0])
    for row, p in ((20, 2.0 ** -3), (60, 2.0 ** 5)):   # the block maximum 7 p fixes 2^E = p: exact ties and saturation
        kv[row, :, 32:64] = 0.0
        kv[row, :, 32:32 + ties.numel()] = ties * p
    kv = kv.to(src_dtype)                # K and V: strided views of one fused buffer
    k, v = kv[:, :HKV], kv[:, HKV:]
    (kq, ks), (vq, vs) = quantize_rows(k), quantize_rows(v)
    n_pages = 3 * HKV * P + 2
    rows = n_pages * PS
    pt = torch.randperm(3 * HKV * P, generator=g).view(3, HKV, P).to(torch.int32)
    bm = torch.tensor([2, 1], dtype=torch.int32)
    cu = torch.tensor([0, 37, 107], dtype=torch.int32)

    def fresh():
        return (torch.full((rows, D // 2), 0x55, dtype=torch.uint8), torch.full((rows, D // 2), 0x55, dtype=torch.uint8),
                torch.full((rows, D // 32), 0xA7, dtype=torch.uint8), torch.full((rows, D // 32), 0xA7, dtype=torch.uint8))

    def check(got, want, what):
        for name, a, b in zip(("k codes", "v codes", "k scale", "v scale"), got, want):
            a = a.cpu()
            if "codes" in name:
                a, b = code_values(a), code_values(b)
            assert torch.equal(a, b), (what, name, int((a != b).sum()))

    kd, vd, pd, bd, cd = k.to(dev), v.to(dev), pt.to(dev), bm.to(dev), cu.to(dev)

    # ---- store every row ----
    want = fresh()
    for b in range(B):
        for h in range(HKV):
            r = O.cache_rows(pt[int(bm[b]), h], seqlens[b], PS)
            sl = slice(int(cu[b]), int(cu[b + 1]))
            want[0][r], want[1][r], want[2][r], want[3][r] = kq[sl, h], vq[sl, h], ks[sl, h], vs[sl, h]
    kc, vc, ksc, vsc = (t.to(dev) for t in fresh())
    lens = torch.zeros(B, HKV, dtype=torch.int32, device=dev)
    prefill_store_all_kv(new_keys=kd, new_values=vd, cu_seqlens_k=cd, max_seqlen_k=70, k_cache=kc, v_cache=vc,
                         page_table=pd, bh_lens=lens, batch_mapping=bd, PAGE_SIZE=PS, k_scale=ksc, v_scale=vsc)
    check((kc, vc, ksc, vsc), want, "store_all")
    assert lens.cpu().tolist() == [[37, 37], [70, 70]]

    # ---- append one row per (b, h); the RESERVED row of the batch is skipped ----
    new = torch.randn(3, 2 * HKV, D, generator=g).to(src_dtype)
    nk, nv = new[:, :HKV], new[:, HKV:]
    (nkq, nks), (nvq, nvs) = quantize_rows(nk), quantize_rows(nv)
    bm3 = torch.tensor([2, RESERVED_BATCH, 1], dtype=torch.int32)
    lens3 = torch.tensor([[37, 37], [5, 5], [70, 70]], dtype=torch.int32)
    for b in (0, 2):
        for h in range(HKV):
            r = int(O.cache_rows(pt[int(bm3[b]), h], int(lens3[b, h]) + 1, PS)[-1])
            want[0][r], want[1][r], want[2][r], want[3][r] = nkq[b, h], nvq[b, h], nks[b, h], nvs[b, h]
    lens3d = lens3.to(dev)
    decode_store_kv(key=nk.to(dev), value=nv.to(dev), batch_mapping=bm3.to(dev), bh_lens=lens3d, page_table=pd,
                    k_cache=kc, v_cache=vc, PAGE_SIZE=PS, k_scale=ksc, v_scale=vsc)
    check((kc, vc, ksc, vsc), want, "decode_store")
    assert lens3d.cpu().tolist() == [[38, 38], [5, 5], [71, 71]]

    # ---- compaction: about half of the rows kept, token order; lengths and kept lists as in the 16-bit path ----
    scores = torch.randn(N, HKV, generator=g).to(dev)
    retain = torch.tensor([37 * HKV // 2, 70 * HKV // 2], dtype=torch.int32, device=dev)

    def compact(kc_, vc_, **scales):
        l0 = torch.zeros(B, HKV, dtype=torch.int32, device=dev)
        return extract_and_store_top_kv(scores, cd, 70, 70 * HKV, HKV, kd, vd, retain, pd, bd, l0, kc_, vc_, PS,
                                        **scales)

    kept16, lens16 = compact(torch.zeros(rows, D, dtype=src_dtype, device=dev),
                             torch.zeros(rows, D, dtype=src_dtype, device=dev))
    kc, vc, ksc, vsc = (t.to(dev) for t in fresh())
    kept, new_lens = compact(kc, vc, k_scale=ksc, v_scale=vsc)
    assert torch.equal(new_lens, lens16)
    want = fresh()
    for b in range(B):
        for h in range(HKV):
            n = int(new_lens[b, h])
            assert torch.equal(kept[b, h, :n], kept16[b, h, :n])
            tok = kept[b, h, :n].cpu().long() + int(cu[b])
            r = O.cache_rows(pt[int(bm[b]), h], n, PS)
            want[0][r], want[1][r], want[2][r], want[3][r] = kq[tok, h], vq[tok, h], ks[tok, h], vs[tok, h]
    check((kc, vc, ksc, vsc), want, "compaction")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,HQ,HKV,D,PS,maxlen", [
    (2, 8, 2, 128, 128, 700),      # G = 4
    (3, 16, 2, 128, 128, 1500),    # G = 8
    (2, 4, 4, 64, 32, 300),        # G = 1, D = 64: one split by default
    (1, 2, 1, 128, 32, 17000),     # more than 512 pages
])
def test_decode_mxfp4_against_float64(dev, dtype, B, HQ, HKV, D, PS, maxlen):
    """Decode attention over e2m1 codes + block scales, with the default plan and with a key_split hint that forces
    more splits, against softmax attention over the dequantised rows in float64.  Every cache byte outside the valid
    rows is 0xFF (stale scales are NaNs) and the lengths are no multiples of 32.  Head (0, 0) is empty and, for B > 1,
    so is the whole of sequence 1: exact zeros.  The single-head shape keeps its one head at full length (it is there
    for the page table wider than the 512-page register window) and also runs as ONE split through the C ABI.
    Afterwards the workspace is all zeros."""
    from compactor_vllm_amd import _lib
    from compactor_vllm_amd.attention import sparse_decode_kernel as dk

    g = torch.Generator().manual_seed(B * 7919 + D + maxlen)
    lens = torch.randint(1, maxlen + 1, (B, HKV), generator=g, dtype=torch.int32)
    lens[-1, -1] = maxlen
    lens[lens % 32 == 0] -= 1
    if B * HKV > 1:
        lens[0, 0] = 0
    if B > 1:
        lens[1, :] = 0
    kf, vf, pt, bm, P = mk_paged(B, HKV, D, PS, lens, torch.float32, seed=3)
    (kq, ks), (vq, vs) = quantize_rows(kf), quantize_rows(vf)
    valid = torch.zeros(kf.shape[0], dtype=torch.bool)
    q = torch.randn(B, HQ, D, generator=g).to(dtype)
    scale = 1.0 / math.sqrt(D)
    G = HQ // HKV
    ref = torch.zeros(B, HQ, D, dtype=torch.float64)
    for b in range(B):
        for h in range(HKV):
            r = O.cache_rows(pt[int(bm[b]), h], int(lens[b, h]), PS)
            valid[r] = True
            if r.numel():
                K, V = dequantize(kq[r], ks[r]), dequantize(vq[r], vs[r])
                p = torch.softmax(q[b, h * G:(h + 1) * G].double() @ K.T * scale, dim=-1)
                ref[b, h * G:(h + 1) * G] = p @ V
    for t in (kq, ks, vq, vs):
        t[~valid] = 0xFF
    dv = [t.to(dev) for t in (q, kq, vq, lens, pt, bm, ks, vs)]
    outs = [dk.head_sparse_decode_attention(dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], HKV, PS, scale, key_split=hint,
                                            k_scale=dv[6], v_scale=dv[7]) for hint in (None, 8)]
    if P > 512:  # one split longer than the page-id window
        o1 = torch.empty_like(dv[0])
        st = _lib.lib().cvllm_decode_attn_mxfp4(
            dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[6].data_ptr(), dv[7].data_ptr(), o1.data_ptr(),
            dv[3].data_ptr(), dv[4].data_ptr(), dv[5].data_ptr(), None, 0, B, HQ, HKV, D, PS, P, scale, 1,
            _lib.dtype_code(dtype), _lib.stream())
        assert st == 0
        outs.append(o1)
    torch.cuda.synchronize()
    for o in outs:
        err = float((o.cpu().double() - ref).abs().max())
        print(f"mxfp4 decode {dtype} B{B} HQ{HQ} HKV{HKV} D{D} PS{PS} L{maxlen}: max abs err {err:.3e}")
        assert torch.allclose(o.cpu().double(), ref, rtol=1e-6, atol=tol(dtype)), err
        if B * HKV > 1:
            assert (o[0, :G] == 0).all()
        if B > 1:
            assert (o[1] == 0).all()
    buf = dk._workspaces.get((dev.index, torch.cuda.current_stream(dev).cuda_stream))
    assert buf is None or int(buf.count_nonzero()) == 0


def _llm(dev, *, eager):
    from compactor_vllm_amd import LLM, LLMConfig

    cfg = TinyConfig()
    conf = LLMConfig(model="tiny", max_num_seqs=8, max_model_len=1024, hf_config=cfg, kvcache_page_size=128,
                     enforce_eager=eager, show_progress_bar=False, kv_cache_dtype="mxfp4")
    return LLM(conf, TinyModel(cfg, dev), device=dev, num_pages=60, max_batched_tokens=2048)


@pytest.mark.parametrize("method_name,ratio", [("COMPACTOR", 0.5), ("NONE", 1.0)])
@pytest.mark.parametrize("eager", [False, True])
def test_engine_mxfp4_mixed_batch_equals_per_request_runs(dev, method_name, ratio, eager):
    """Block quantisation is batch invariant: an 8-request mixed batch on an MXFP4 cache equals per-request runs token
    for token; every page and batch row is free afterwards; prefix registration is refused."""
    from compactor_vllm_amd import BatchCompressionParams, CompressionMethod, SamplingParams, SequenceCompressionParams

    g = torch.Generator().manual_seed(11)
    plens = [700, 33, 257] + [int(x) for x in torch.randint(40, 700, (5,), generator=g)]
    prompts = [torch.randint(0, 512, (n,), generator=g).tolist() for n in plens]
    sp = [SamplingParams(temperature=0.0, max_new_tokens=int(x)) for x in torch.randint(1, 16, (8,), generator=g)]
    bcp = BatchCompressionParams(compression_method=CompressionMethod[method_name])
    scp = lambda: SequenceCompressionParams(ratio, protected_first_tokens=4, protected_last_tokens=16)  # noqa: E731
    llm = _llm(dev, eager=eager)
    mgr = llm.master_model_runner.kv_manager
    assert mgr.paged_cache.kv_cache.dtype == torch.uint8 and mgr.paged_cache.kv_scale.dtype == torch.uint8
    out = llm.generate(prompts, sp, bcp, per_sequence_compression_params=[scp() for _ in prompts])
    assert mgr.num_free_batches == 8 and mgr.num_free_pages == 60
    solo = _llm(dev, eager=eager)
    for i, (p, s) in enumerate(zip(prompts, sp)):
        assert solo.generate([p], s, bcp, per_sequence_compression_params=scp())[0] == out[i], (i, len(p))
    with pytest.raises(NotImplementedError):
        llm.master_model_runner.cache_prefix(prompts[0], bcp)
    torch.cuda.synchronize()
