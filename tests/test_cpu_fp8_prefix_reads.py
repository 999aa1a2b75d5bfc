"""CPU: `LLMConfig.fp8_prefix_reads` - the opt-in that lets prefill attention read an FP8 prefix (chunked prefill, prefix
reuse on an FP8 cache)."""
import pytest

from tiny_model import TinyConfig


@pytest.mark.parametrize("kv_dtype,flag,chunked,reads", [("fp8_e4m3", False, False, False), ("fp8_e4m3", True, True, True),
                                                         ("auto", True, True, False)])
def test_fp8_prefix_reads_switches_chunked_prefill(kv_dtype, flag, chunked, reads):
    from compactor_vllm_amd import LLMConfig, _lib
    from compactor_vllm_amd.core.memory_manager import KVCacheManager

    assert LLMConfig(model="tiny", hf_config=TinyConfig()).fp8_prefix_reads is False
    conf = LLMConfig(model="tiny", hf_config=TinyConfig(), kvcache_page_size=128, kv_cache_dtype=kv_dtype,
                     fp8_prefix_reads=flag)
    mgr = KVCacheManager(conf, "cpu", num_pages=4)
    assert (mgr.chunked_prefill, mgr.fp8_prefix_reads) == (chunked, reads)
    assert {"cvllm_prefill_attn_fp8", "cvllm_compact_cache_inplace_fp8"} <= set(_lib.SIGNATURES)
