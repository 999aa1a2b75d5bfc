"""CPU: cvllm_snapkv_scores_paged is exported and refuses bad arguments before any launch (no GPU is touched)."""
import pytest

ARG, SHAPE = -1, -2
P = 0x1000  # any non-null address: a refused call never dereferences it


def _call(**kw):
    from compactor_vllm_amd import _lib

    a = dict(q=P, k=P, sq_n=1024, sk_n=1024, sk_h=128, k_cache=P, k_scale=None, page_table=P, batch_mapping=P,
             scores=P, cu_q=P, cu_new=P, cu_k=P, window_b=None, B=1, HQ=8, HKV=2, D=128, w=32, sm_scale=0.1, pool=5,
             pool_tile=128, max_seqlen_k=1024, page_size=128, nlp=8, cache_fp8=0, dtype=1, ws=P, ws_bytes=1 << 30,
             stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return _lib.lib().cvllm_snapkv_scores_paged(*a.values())


def test_symbol_is_exported_and_declared():
    from compactor_vllm_amd import _lib

    assert "cvllm_snapkv_scores_paged" in _lib.SIGNATURES and hasattr(_lib.lib(), "cvllm_snapkv_scores_paged")


@pytest.mark.parametrize("kw,status", [
    (dict(q=None), ARG), (dict(k=None), ARG), (dict(k_cache=None), ARG), (dict(page_table=None), ARG),
    (dict(batch_mapping=None), ARG), (dict(scores=None), ARG), (dict(cu_new=None), ARG),
    (dict(cache_fp8=1, k_scale=None), ARG), (dict(page_size=0), ARG),
    (dict(pool_tile=48), SHAPE), (dict(HQ=16, w=33), SHAPE), (dict(D=256), SHAPE), (dict(HQ=6), SHAPE),
])
def test_bad_arguments_are_refused_before_any_launch(kw, status):
    assert _call(**kw) == status
