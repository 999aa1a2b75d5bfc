"""Engine configuration types (`compactor_vllm/config/engine_config.py:9-94`).

`LLMConfig` keeps every field and default of the reference.  The one behavioural difference: when
`hf_config` is None the reference calls `AutoConfig.from_pretrained(model)` (a network fetch); this
build only does so when `transformers` can resolve the name locally, and otherwise raises — always
pass a locally built `hf_config` (there is no network on the target machines).
"""
import os
from dataclasses import dataclass
from enum import Enum, auto
from typing import Any, Optional


class AttentionBackend(Enum):
    FLASH_ATTENTION = auto()
    COMPACTOR_TRITON = auto()  # name kept for drop-in compatibility: here it selects the HIP kernels


@dataclass
class LLMConfig:
    model: str
    path: Optional[str] = None
    nccl_port: Optional[int] = 1218
    max_num_seqs: int = 256
    max_model_len: int = 40960
    gpu_memory_utilization: float = 0.9
    tensor_parallel_size: int = 1
    enforce_eager: bool = False
    hf_config: Any | None = None
    eos: int = -1
    kvcache_page_size: int = 128
    leverage_sketch_size: int = 48
    attention_backend: AttentionBackend = AttentionBackend.COMPACTOR_TRITON
    show_progress_bar: bool = True
    # "auto" = the model dtype; "fp8_e4m3" = e4m3 codes + one fp32 scale per cache row; "mxfp4" = OCP e2m1 codes + one
    # e8m0 scale per 32 elements
    kv_cache_dtype: str = "auto"
    # FP8 cache only: prefill attention reads the FP8 prefix (cvllm_prefill_attn_fp8), which turns chunked prefill and
    # prefix reuse on.  Opt-in for now; without it an FP8 cache refuses both, as before.
    fp8_prefix_reads: bool = False
    # MXFP4 cache only, the same switch: prefill attention reads the 4-bit prefix (cvllm_prefill_attn_mxfp4).  Without it an
    # MXFP4 cache has no chunked prefill and no prefix reuse.  SnapKV scoring does not read 4-bit rows: with it a chunked
    # prompt or a prefix hit raises NotImplementedError.
    mxfp4_prefix_reads: bool = False

    def __post_init__(self):
        if self.kv_cache_dtype not in ("auto", "fp8_e4m3", "mxfp4"):
            raise ValueError(f"kv_cache_dtype must be 'auto', 'fp8_e4m3' or 'mxfp4', got {self.kv_cache_dtype!r}")
        if self.path is not None and not os.path.isdir(self.path):
            raise NotADirectoryError(f"Engine config dir {self.path} does not exist")
        if self.tensor_parallel_size <= 0 or self.tensor_parallel_size > 8:
            raise ValueError("tensor_parallel_size must be >= 1 and <= 8")
        if self.hf_config is None:
            from transformers import AutoConfig

            self.hf_config = AutoConfig.from_pretrained(self.model, local_files_only=True)
        self.max_model_len = min(self.max_model_len, self.hf_config.max_position_embeddings)
