"""CPU: the host side of the MXFP4 KV cache - configuration, cache sizing, the cache object's tensors, and the four C
entry points refusing bad arguments before any launch (no GPU is touched)."""
import pytest
import torch

from tiny_model import TinyConfig

ARG, SHAPE = -1, -2
P = 0x1000  # any non-null address: a refused call never dereferences it


def _config(**kw):
    from compactor_vllm_amd import LLMConfig

    return LLMConfig(model="tiny", hf_config=TinyConfig(), kvcache_page_size=128, **kw)


def test_config_page_bytes_and_chunking():
    from compactor_vllm_amd.core.memory_manager import KVCacheManager

    assert _config(kv_cache_dtype="mxfp4").kv_cache_dtype == "mxfp4"
    with pytest.raises(ValueError):
        _config(kv_cache_dtype="mxfp6")
    cfg = TinyConfig()
    mgr = KVCacheManager(_config(kv_cache_dtype="mxfp4"), "cpu", num_pages=4)
    L, PS, D = cfg.num_hidden_layers, 128, cfg.head_dim
    assert mgr.bytes_per_page_all_layers() == L * 2 * PS * (D // 2 + D // 32)
    assert mgr.cache_dtype == torch.uint8 and not mgr.chunked_prefill


def test_paged_cache_shapes():
    from compactor_vllm_amd.kv_cache.page_table import PagedKVCache

    c = PagedKVCache(num_layers=2, max_logical_pages_per_head=3, num_pages=6, page_size=32, H_kv=2, head_dim=64,
                     max_num_batches=2, device="cpu", dtype=torch.uint8)
    assert c.kv_cache.shape == (2, 2, 6 * 32, 32) and c.kv_cache.dtype == torch.uint8
    assert c.kv_scale.shape == (2, 2, 6 * 32, 2) and c.kv_scale.dtype == torch.uint8
    assert c.layer_slices(1)[0].shape == (6 * 32, 32)
    ks, vs = c.layer_scale_slices(1)
    assert ks.shape == (6 * 32, 2) and ks.data_ptr() != vs.data_ptr()
    row = c.new_batch()
    c.reserve_tokens(row, 96)  # 3 pages per (layer, head)
    assert c.reclaim_pages(row) == 2 * 2 * 3 * 32 * (32 + 2) * 2  # K + V codes and their scales


def _store(name, **kw):
    from compactor_vllm_amd import _lib

    lists = {
        "cvllm_store_decode_kv_mxfp4": dict(key=P, value=P, sk_b=256, sk_h=128, sv_b=256, sv_h=128, bm=P, lens=P, pt=P,
                                            kc=P, vc=P, B=1, HKV=2, D=128, ps=32, nlp=4, reserved=0, dtype=1,
                                            stream=None, ks=P, vs=P),
        "cvllm_store_all_kv_mxfp4": dict(key=P, value=P, sk_b=256, sk_h=128, sv_b=256, sv_h=128, cu=P, bm=P, lens=P,
                                         pt=P, kc=P, vc=P, B=1, N=8, HKV=2, D=128, ps=32, nlp=4, dtype=1, stream=None,
                                         ks=P, vs=P),
        "cvllm_compact_store_mxfp4": dict(key=P, value=P, sk_b=256, sk_h=128, sv_b=256, sv_h=128, kept=P, new_lens=P,
                                          cu=P, lens=P, pt=P, bm=P, kc=P, vc=P, B=1, HKV=2, D=128, max_seqlen=8, ps=32,
                                          nlp=4, dtype=1, stream=None, ks=P, vs=P),
        "cvllm_decode_attn_mxfp4": dict(key=P, kc=P, vc=P, ks=P, vs=P, out=P, lens=P, pt=P, bm=P, ws=None, ws_bytes=0,
                                        B=1, HQ=8, HKV=2, D=128, ps=32, nlp=4, sm_scale=0.1, n_splits=1, dtype=1,
                                        stream=None),
    }
    a = lists[name]
    assert set(kw) <= set(a)
    a.update(kw)
    return getattr(_lib.lib(), name)(*a.values())


NAMES = ["cvllm_store_decode_kv_mxfp4", "cvllm_store_all_kv_mxfp4", "cvllm_compact_store_mxfp4",
         "cvllm_decode_attn_mxfp4"]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kw,status", [(dict(key=None), ARG), (dict(kc=None), ARG), (dict(vc=None), ARG),
                                       (dict(ks=None), ARG), (dict(vs=None), ARG), (dict(pt=None), ARG),
                                       (dict(D=256), SHAPE), (dict(dtype=2), SHAPE)])
def test_bad_arguments_are_refused_before_any_launch(name, kw, status):
    from compactor_vllm_amd import _lib

    assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _store(name, **kw) == status


@pytest.mark.parametrize("kw", [dict(HQ=6), dict(HQ=32), dict(ps=48)])
def test_decode_refuses_bad_shapes(kw):
    assert _store("cvllm_decode_attn_mxfp4", **kw) == SHAPE
