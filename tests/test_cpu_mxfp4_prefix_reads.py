"""CPU: `LLMConfig.mxfp4_prefix_reads` - the opt-in that lets prefill attention read an MXFP4 prefix (chunked prefill,
prefix reuse on an MXFP4 cache) - and the two C entry points behind it refusing bad arguments before any launch."""
import pytest

from tiny_model import TinyConfig

ARG, SHAPE = -1, -2
P = 0x1000  # any non-null address: a refused call never dereferences it


@pytest.mark.parametrize("kv_dtype,flag,chunked,reads", [("mxfp4", False, False, False), ("mxfp4", True, True, True),
                                                         ("auto", True, True, False)])
def test_mxfp4_prefix_reads_switches_chunked_prefill(kv_dtype, flag, chunked, reads):
    from compactor_vllm_amd import LLMConfig
    from compactor_vllm_amd.core.memory_manager import KVCacheManager

    assert LLMConfig(model="tiny", hf_config=TinyConfig()).mxfp4_prefix_reads is False
    conf = LLMConfig(model="tiny", hf_config=TinyConfig(), kvcache_page_size=128, kv_cache_dtype=kv_dtype,
                     mxfp4_prefix_reads=flag)
    mgr = KVCacheManager(conf, "cpu", num_pages=4)
    assert (mgr.chunked_prefill, mgr.mxfp4_prefix_reads) == (chunked, reads)


def _call(name, **kw):
    from compactor_vllm_amd import _lib

    lists = {
        "cvllm_prefill_attn_mxfp4": dict(q=P, k=P, v=P, sq_n=1024, sk_n=256, sk_h=128, sv_n=256, sv_h=128, kc=P, vc=P,
                                         out=P, lens=P, pt=P, bm=P, cu=P, B=1, N=8, max_q=8, HQ=8, HKV=2, D=128, ps=32,
                                         nlp=4, sm_scale=0.1, dtype=1, stream=None, ks=P, vs=P),
        "cvllm_compact_cache_inplace_mxfp4": dict(kept=P, new_lens=P, dst=P, src=P, pt=P, bm=P, kc=P, vc=P, B=1, H=2,
                                                  D=128, max_seqlen=8, ps=32, nlp=4, stream=None, ks=P, vs=P),
    }
    a = lists[name]
    assert name in _lib.SIGNATURES and set(kw) <= set(a)
    a.update(kw)
    return getattr(_lib.lib(), name)(*a.values())


@pytest.mark.parametrize("name,kw,status", [
    *[(n, {key: None}, ARG) for n in ("cvllm_prefill_attn_mxfp4", "cvllm_compact_cache_inplace_mxfp4")
      for key in ("kc", "vc", "ks", "vs", "pt", "bm")],
    ("cvllm_prefill_attn_mxfp4", dict(q=None), ARG), ("cvllm_prefill_attn_mxfp4", dict(cu=None), ARG),
    ("cvllm_compact_cache_inplace_mxfp4", dict(kept=None), ARG),
    ("cvllm_prefill_attn_mxfp4", dict(D=256), SHAPE), ("cvllm_prefill_attn_mxfp4", dict(dtype=2), SHAPE),
    ("cvllm_prefill_attn_mxfp4", dict(HQ=6), SHAPE), ("cvllm_prefill_attn_mxfp4", dict(HQ=32), SHAPE),
    ("cvllm_compact_cache_inplace_mxfp4", dict(D=256), SHAPE),
])
def test_bad_arguments_are_refused_before_any_launch(name, kw, status):
    assert _call(name, **kw) == status
