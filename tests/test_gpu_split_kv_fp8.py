"""GPU: split-KV decode shards on an FP8 (e4m3) cache and the append rank's one-launch step (fused append + LSE) on both
cache types, against float64 softmax attention over the dequantised rows, float(code) * scale."""
import math

import pytest
import torch

from compactor_vllm_amd.attention import sparse_decode_kernel as dk
from compactor_vllm_amd.attention.cross_gpu_decode import merge_shards, split_kv_decode_attention
from compactor_vllm_amd.kv_cache.store_kv_cache import decode_store_kv
from helpers import mk_paged, tol
from oracle import ref_cpu as O
from test_gpu_split_kv import _shard

pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])]


def quantize_rows(x):  # x [..., D] fp32 -> (e4m3 codes, fp32 scale); tensor / tensor = IEEE divisions
    a = x.abs().amax(dim=-1).clamp_min(1e-30)
    c448 = torch.full_like(a, 448.0)
    return (x * (c448 / a)[..., None]).to(torch.float8_e4m3fn), a / c448


def _fp8_cache(B, HKV, D, PS, lens, seed):  # CPU: (k codes, k scales, v codes, v scales, page table, batch mapping)
    kf, vf, pt, bm, _ = mk_paged(B, HKV, D, PS, lens, torch.float32, seed=seed)
    return (*quantize_rows(kf), *quantize_rows(vf), pt, bm)


def _ref64(q, kc, ks, vc, vs, pt, bm, lens, PS, new=None):
    """(out [B,HQ,D], lse [B,HQ]) in float64 over the dequantised rows, then the rows new = (K, V) [B,HKV,D]"""
    (B, HQ, D), HKV = q.shape, lens.shape[1]
    out, lse = torch.zeros(B, HQ, D, dtype=torch.float64), torch.full((B, HQ), -math.inf, dtype=torch.float64)
    for b in range(B):
        for h in range(HKV):
            r, hq = O.cache_rows(pt[int(bm[b]), h], int(lens[b, h]), PS), slice(h * HQ // HKV, (h + 1) * HQ // HKV)
            K, V = kc[r].double() * ks[r].double()[:, None], vc[r].double() * vs[r].double()[:, None]
            if new is not None:
                K, V = torch.cat([K, new[0][b, h][None]]), torch.cat([V, new[1][b, h][None]])
            if len(K):  # no rows: zeros and -inf
                s = q[b, hq].double() @ K.T / math.sqrt(D)
                lse[b, hq], out[b, hq] = torch.logsumexp(s, -1), torch.softmax(s, -1) @ V
    return out, lse


def _close_lse(lse, ref):  # the 16-bit shard test's bound: the same finite mask, rtol 1e-4, atol 1e-3
    fin = torch.isfinite(ref)
    assert torch.equal(fin, torch.isfinite(lse))
    assert torch.allclose(lse[fin].double(), ref[fin].double(), rtol=1e-4, atol=1e-3), (lse[fin] - ref[fin]).abs().max()


@pytest.mark.parametrize("B,HQ,HKV,D,PS,maxlen,W,key_split", [
    (2, 8, 2, 128, 128, 700, 2, None),   # 3 splits: stage-2 LSE; a head of length 0; one inside a single page
    (40, 8, 2, 64, 32, 300, 2, None),    # 80 (b,h) groups: one split each, the kernel's own LSE write; D = 64
    (1, 16, 2, 128, 128, 3000, 3, 8),    # G = 8, forced splits, 3 shards
])
def test_fp8_shards_merge_to_full_attention(dev, dtype, B, HQ, HKV, D, PS, maxlen, W, key_split):
    g = torch.Generator().manual_seed(B + maxlen + W)
    lens = torch.randint(1, maxlen + 1, (B, HKV), generator=g, dtype=torch.int32)
    lens[0, 0], lens[-1, -1] = maxlen, PS // 2  # the short one: every shard but one holds nothing of this head
    if B > 1:
        lens[1, 0] = 0  # nobody holds anything
    *cache, pt, bm = _fp8_cache(B, HKV, D, PS, lens, 3)
    q = torch.randn(B, HQ, D, generator=g).to(dtype)
    kc, ks, vc, vs = [t.to(dev) for t in cache]
    outs, lses = [], []
    for r in range(W):
        my_pt, my_lens = _shard(pt, bm, lens, PS, W, r)
        o, l = dk.head_sparse_decode_attention(q.to(dev), kc, vc, my_lens.to(dev), my_pt.to(dev), bm.to(dev), HKV, PS,
                                               key_split=key_split, return_lse=True, k_scale=ks, v_scale=vs)
        o_ref, l_ref = _ref64(q, *cache, my_pt, bm, my_lens, PS)
        _close_lse(l.cpu(), l_ref)
        assert torch.allclose(o.cpu().double(), o_ref, atol=tol(dtype))
        assert (o.cpu()[~torch.isfinite(l_ref)] == 0).all()
        outs.append(o)
        lses.append(l)
    merged = merge_shards(torch.stack(outs), torch.stack(lses)).cpu().double()
    ref = _ref64(q, *cache, pt, bm, lens, PS)[0]
    assert torch.allclose(merged, ref, atol=tol(dtype)), (merged - ref).abs().max()
    assert all(int(buf.count_nonzero()) == 0 for buf in dk._workspaces.values())


@pytest.mark.parametrize("fp8", [True, False])
@pytest.mark.parametrize("B,HQ,HKV,D,PS", [(3, 8, 2, 128, 128), (40, 8, 2, 64, 32)])
def test_fused_append_lse_equals_store_then_attend(dev, dtype, fp8, B, HQ, HKV, D, PS):
    """Caches, scales, lengths and the live outputs bit-equal; lse bit-equal on FP8, within the shard bound on 16-bit.
    B = 3: two splits, every old length a unit or page boundary, all rows live.  B = 40: one split; sequence 5 sits
    on the RESERVED row (0): lse -inf, zero output, nothing stored (the caches equal the store path's, which skips it)."""
    lens = torch.randint(0, 300, (B * HKV,), generator=torch.Generator().manual_seed(B), dtype=torch.int32)
    lens[:6] = torch.tensor([0, 31, 32, 127, 128, 600 if B == 3 else 299], dtype=torch.int32)
    lens = lens.view(B, HKV)
    kc, ks, vc, vs, pt, bm = _fp8_cache(B, HKV, D, PS, lens + 1, 5)
    live = torch.ones(B, dtype=torch.bool)
    if B > 3:
        bm[5], live[5] = 0, False
    if not fp8:
        kc, vc = (kc.float() * ks[:, None]).to(dtype), (vc.float() * vs[:, None]).to(dtype)
    table = torch.full((pt.shape[0], HKV), 3, dtype=torch.int32)
    table[bm.long()] = lens
    qkv = torch.randn(B, HQ + 2 * HKV, D, generator=torch.Generator().manual_seed(D)).to(dtype)
    res = []
    for fused in (False, True):
        q, k, v, c_k, c_v, tb, ptd, bmd, *sc = [t.to(dev) for t in (qkv[:, :HQ].contiguous(), qkv[:, HQ:HQ + HKV],
                                                qkv[:, HQ + HKV:], kc, vc, table, pt, bm, *([ks, vs] if fp8 else []))]
        sc = dict(zip(("k_scale", "v_scale"), sc))
        if fused:
            out, lse = dk.fused_decode_step(q, k, v, c_k, c_v, tb, ptd, bmd, HKV, PS, return_lse=True, **sc)
        else:
            seq = tb.index_select(0, bmd.long()).contiguous()
            decode_store_kv(key=k, value=v, batch_mapping=bmd, bh_lens=seq, page_table=ptd, k_cache=c_k, v_cache=c_v,
                            PAGE_SIZE=PS, **sc)
            out, lse = dk.head_sparse_decode_attention(q, c_k, c_v, seq, ptd, bmd, HKV, PS, return_lse=True, **sc)
            tb.index_copy_(0, bmd.long(), seq)
        res.append([t.cpu() for t in (c_k.view(torch.uint8), c_v.view(torch.uint8), tb, out[live.to(dev)], *sc.values(), lse)])
    for i, (x, y) in enumerate(zip(res[0][:-1], res[1][:-1])):
        assert torch.equal(x, y), (i, int((x != y).sum()))
    assert torch.equal(res[1][2][bm[live].long()], lens[live] + 1)
    if fp8:
        assert torch.equal(res[0][-1][live], res[1][-1][live])
    else:
        _close_lse(res[1][-1][live], res[0][-1][live])
    assert (res[1][-1][~live] == -math.inf).all() and (out.cpu()[~live] == 0).all()


def test_split_kv_step_fp8_one_process(dev, dtype, monkeypatch):
    """split_kv_decode_attention once per shard (world size 1, the gather a copy), rank 0 appending; merged afterwards."""
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 1)
    monkeypatch.setattr(torch.distributed, "all_gather_into_tensor", lambda out, inp, group=None: out.copy_(inp))
    B, HQ, HKV, D, PS, W = 2, 8, 2, 128, 128, 2
    lens = torch.tensor([[700, 128], [0, 333]], dtype=torch.int32)
    *cache, pt, bm = _fp8_cache(B, HKV, D, PS, lens + PS, 7)  # lens + PS: a spare page behind every head
    kc, ks, vc, vs = [t.to(dev) for t in cache]
    qkv = torch.randn(B, HQ + 2 * HKV, D, generator=torch.Generator().manual_seed(1)).to(dtype)
    q, key, val = qkv[:, :HQ].contiguous(), qkv[:, HQ:HQ + HKV], qkv[:, HQ + HKV:]
    pairs = []
    for r in range(W):
        my_pt, my_lens = _shard(pt, bm, lens, PS, W, r)
        kw = {}
        if r == 0:  # the append rank: the spare page follows its slice; its lengths live in a layer table
            for b in range(B):
                for h in range(HKV):
                    my_pt[int(bm[b]), h, -(-int(my_lens[b, h]) // PS)] = pt[int(bm[b]), h, -(-int(lens[b, h]) // PS)]
            table, lens0 = torch.zeros(pt.shape[0], HKV, dtype=torch.int32), my_lens
            table[bm.long()] = my_lens
            table = table.to(dev)
            kw = dict(key=key.to(dev), value=val.to(dev), bh_seq_lens_layer=table)
        split_kv_decode_attention(q.to(dev), kc, vc, my_lens.to(dev), my_pt.to(dev), bm.to(dev), HKV, PS, None, None,
                                  k_scale=ks, v_scale=vs, merge=lambda o, l: pairs.append((o[0], l[0])), **kw)
    merged = merge_shards(torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])).cpu().double()
    new = [c.double() * s.double()[..., None] for c, s in (quantize_rows(key.float()), quantize_rows(val.float()))]
    ref = _ref64(q, *cache, pt, bm, lens, PS, new=new)[0]
    assert torch.allclose(merged, ref, atol=tol(dtype)), (merged - ref).abs().max()
    assert torch.equal(table.cpu()[bm.long()], lens0 + 1)
