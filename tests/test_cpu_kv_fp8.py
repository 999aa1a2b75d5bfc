"""CPU: the host side of the FP8 (e4m3) KV cache - configuration, cache sizing and the cache object's scale tensor."""
import pytest
import torch

from tiny_model import TinyConfig


def _config(**kw):
    from compactor_vllm_amd import LLMConfig

    return LLMConfig(model="tiny", hf_config=TinyConfig(), kvcache_page_size=128, **kw)


def test_kv_cache_dtype_is_validated():
    assert _config().kv_cache_dtype == "auto"
    assert _config(kv_cache_dtype="fp8_e4m3").kv_cache_dtype == "fp8_e4m3"
    with pytest.raises(ValueError):
        _config(kv_cache_dtype="int3")


@pytest.mark.parametrize("kv_dtype", ["auto", "fp8_e4m3"])
def test_page_bytes_and_chunking(kv_dtype):
    from compactor_vllm_amd.core.memory_manager import KVCacheManager

    cfg = TinyConfig()
    mgr = KVCacheManager(_config(kv_cache_dtype=kv_dtype), "cpu", num_pages=4)
    L, PS, D = cfg.num_hidden_layers, 128, cfg.head_dim
    if kv_dtype == "auto":
        assert mgr.bytes_per_page_all_layers() == L * 2 * PS * D * 2 and mgr.chunked_prefill
    else:
        assert mgr.bytes_per_page_all_layers() == L * 2 * PS * (D + 4) and not mgr.chunked_prefill


def test_paged_cache_carries_scales():
    from compactor_vllm_amd.kv_cache.page_table import PagedKVCache

    kw = dict(num_layers=2, max_logical_pages_per_head=3, num_pages=6, page_size=32, H_kv=2, head_dim=64,
              max_num_batches=2, device="cpu")
    fp8 = PagedKVCache(dtype=torch.float8_e4m3fn, **kw)
    assert fp8.kv_scale.shape == (2, 2, 6 * 32) and fp8.kv_scale.dtype == torch.float32
    assert fp8.kv_cache.element_size() == 1 and len(fp8.layer_slices(1)) == 4
    ks, vs = fp8.layer_scale_slices(1)
    assert ks.shape == (6 * 32,) and ks.data_ptr() != vs.data_ptr()
    row = fp8.new_batch()
    fp8.reserve_tokens(row, 96)  # 3 pages per (layer, head)
    assert fp8.reclaim_pages(row) == 2 * 2 * 3 * 32 * (64 + 4) * 2  # K + V codes and their scales
    plain = PagedKVCache(dtype=torch.bfloat16, **kw)
    assert plain.kv_scale is None and plain.layer_scale_slices(0) == (None, None)
