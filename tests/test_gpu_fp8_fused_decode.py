"""GPU: the fused decode step on an FP8 (e4m3) cache (quantising append + attention in one launch) against the
four-call sequence bit for bit, against float64, with a page table wider than the page-id window, and in the layer."""
import functools
import math

import pytest
import torch

from helpers import mk_paged, tol
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
SHAPES = [(8, 2, 128, 128), (16, 2, 128, 32), (4, 4, 64, 32)]  # HQ, HKV, D, PS: G = 4, 8, 1
LIVE = [0, 2, 3]  # row 1 of the batch of 4 maps to RESERVED_BATCH


def quantize_rows(x):  # x [..., D] fp32 -> (e4m3 codes, fp32 scale); tensor / tensor = IEEE divisions
    a = x.abs().amax(dim=-1).clamp_min(1e-30)
    c448 = torch.full_like(a, 448.0)
    return (x * (c448 / a)[..., None]).to(torch.float8_e4m3fn), a / c448


def _corner_lens(HKV, PS):  # old lengths [4, HKV]: the live rows' first six pinned to the corners, the rest random
    lens = torch.randint(1, 700, (4 * HKV,), generator=torch.Generator().manual_seed(PS + HKV), dtype=torch.int32)
    lens[:6] = torch.tensor([0, 31, 32, PS - 1, PS, 2 * PS + 1], dtype=torch.int32)
    return lens.view(4, HKV)[[0, 3, 1, 2]].contiguous()


def _setup(dtype, HQ, HKV, D, PS, lens_old, reserved_row=None):
    """CPU tensors: a quantised cache with one free slot per head (stale codes in it), the layer's length table, the new
    token with key / value as strided views of one fused buffer."""
    from compactor_vllm_amd.config.constants import RESERVED_BATCH

    kf, vf, pt, bm, _ = mk_paged(lens_old.shape[0], HKV, D, PS, lens_old + 1, torch.float32, seed=5)
    if reserved_row is not None:
        bm[reserved_row] = RESERVED_BATCH
    (kc, ks), (vc, vs) = quantize_rows(kf), quantize_rows(vf)
    table = torch.full((pt.shape[0], HKV), 3, dtype=torch.int32)
    table[bm.long()] = lens_old
    qkv = torch.randn(lens_old.shape[0], HQ + 2 * HKV, D, generator=torch.Generator().manual_seed(D)).to(dtype)
    return dict(q=qkv[:, :HQ].contiguous(), k=qkv[:, HQ:HQ + HKV], v=qkv[:, HQ + HKV:], kc=kc, vc=vc, ks=ks, vs=vs,
                table=table, pt=pt, bm=bm, lens=lens_old)


def _step(dev, cpu, HKV, PS, key_split, fused):
    """One decode step on a fresh device copy, fused or as the four calls (key_split "layer": both through
    Attention.forward); returns [k codes, v codes, k scale, v scale, length table, out] on the CPU."""
    from compactor_vllm_amd.attention import sparse_decode_kernel as dk
    from compactor_vllm_amd.kv_cache.store_kv_cache import decode_store_kv
    from compactor_vllm_amd.layers.attention import Attention
    from compactor_vllm_amd.utils.context import reset_context, set_context

    d = {k: t.to(dev) for k, t in cpu.items()}
    sc = dict(k_scale=d["ks"], v_scale=d["vs"])
    if key_split == "layer":
        attn = Attention(d["q"].shape[1], d["q"].shape[2], 1.0 / math.sqrt(d["q"].shape[2]), HKV)
        attn.fused_decode, attn.page_size, attn.page_table, attn.bh_seq_lens = fused, PS, d["pt"], d["table"]
        attn.k_cache, attn.v_cache, attn.k_scale, attn.v_scale = d["kc"], d["vc"], d["ks"], d["vs"]
        set_context(is_prefill=False, batch_mapping=d["bm"])  # the default length hint: both plans use the same S
        out = attn(d["q"], d["k"], d["v"])
        reset_context()
    elif fused:
        out = dk.fused_decode_step(d["q"], d["k"], d["v"], d["kc"], d["vc"], d["table"], d["pt"], d["bm"], HKV, PS,
                                   key_split=key_split, **sc)
    else:
        seq = d["table"].index_select(0, d["bm"].long()).contiguous()
        decode_store_kv(key=d["k"], value=d["v"], batch_mapping=d["bm"], bh_lens=seq, page_table=d["pt"],
                        k_cache=d["kc"], v_cache=d["vc"], PAGE_SIZE=PS, **sc)
        out = dk.head_sparse_decode_attention(d["q"], d["kc"], d["vc"], seq, d["pt"], d["bm"], HKV, PS,
                                              key_split=key_split, **sc)
        d["table"].index_copy_(0, d["bm"].long(), seq)
    return [d[n].view(torch.uint8).cpu() for n in ("kc", "vc")] + [t.cpu() for t in (d["ks"], d["vs"], d["table"], out)]


@functools.lru_cache(maxsize=None)
def _both(dev, dtype, shape, key_split):
    cpu = _setup(dtype, *shape, _corner_lens(shape[1], shape[3]), reserved_row=1)
    return [_step(dev, cpu, shape[1], shape[3], key_split, fused) for fused in (False, True)] + [cpu]


def _assert_same(sa, sb, cpu, live):
    for i, (x, y) in enumerate(zip(sa[:5] + [sa[5][live]], sb[:5] + [sb[5][live]])):
        assert torch.equal(x, y), ("k codes|v codes|k scale|v scale|lengths|out".split("|")[i], int((x != y).sum()))
    assert torch.equal(sb[4][cpu["bm"][live].long()], cpu["lens"][live] + 1)


@pytest.mark.parametrize("key_split", [None, 8, "layer"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fused_equals_store_then_attend(dev, dtype, shape, key_split):
    """Codes over the whole cache, both scale arrays, the length table and the live rows' outputs are the four-call
    sequence's, bit for bit; the RESERVED row stores nothing and outputs exact zeros.  Old lengths pinned to 0, 31, 32,
    PS-1, PS, 2 PS + 1; with two kv-heads the default plan is ONE split (the kernel publishes the length itself).
    "layer": Attention.forward in decode mode with fused_decode True against False."""
    sa, sb, cpu = _both(dev, dtype, shape, key_split)
    _assert_same(sa, sb, cpu, LIVE)
    assert (sb[5][1] == 0).all()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fused_against_float64(dev, dtype, shape):
    """The fused outputs against softmax attention in float64 over the dequantised rows, the appended one included."""
    HQ, HKV, D, PS = shape
    _, sb, c = _both(dev, dtype, shape, None)
    (nk, nks), (nv, nvs) = quantize_rows(c["k"].float()), quantize_rows(c["v"].float())
    deq = lambda codes, s: codes.double() * s.double()[..., None]  # noqa: E731
    for b in LIVE:
        for h in range(HKV):
            r = O.cache_rows(c["pt"][int(c["bm"][b]), h], int(c["lens"][b, h]), PS)
            K = torch.cat([deq(c["kc"][r], c["ks"][r]), deq(nk[b, h], nks[b, h])[None]])
            V = torch.cat([deq(c["vc"][r], c["vs"][r]), deq(nv[b, h], nvs[b, h])[None]])
            hq = slice(h * HQ // HKV, (h + 1) * HQ // HKV)
            ref = torch.softmax(c["q"][b, hq].double() @ K.T / math.sqrt(D), dim=-1) @ V
            print(f"fp8 fused decode {dtype} D{D} L_old {int(c['lens'][b, h])}: max abs err "
                  f"{float((sb[5][b, hq].double() - ref).abs().max()):.3e}")
            assert torch.allclose(sb[5][b, hq].double(), ref, rtol=1e-6, atol=tol(dtype))


def test_fused_wide_page_table_one_split(dev, monkeypatch):
    """More than 512 pages and n_splits = 1 at the C ABI: the appended row lies beyond the first page-id window."""
    from compactor_vllm_amd.attention import sparse_decode_kernel as dk

    monkeypatch.setattr(dk, "plan_internal_splits", lambda n_bh, bound, key_split: 1)
    cpu = _setup(torch.bfloat16, 2, 1, 128, 32, torch.tensor([[17000]], dtype=torch.int32))
    assert cpu["pt"].shape[-1] > 512
    _assert_same(*(_step(dev, cpu, 1, 32, None, fused) for fused in (False, True)), cpu, [0])
