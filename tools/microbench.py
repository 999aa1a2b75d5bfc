"""Kernel micro-benchmarks on one MI355X (HIP-event timed on the launch stream).

    python tools/microbench.py decode [--L 16384] [--B 1] [--splits 0]
    python tools/microbench.py decode --step [--lse] [--kv-dtype fp8] [--L 16640] [--B 1]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "compactor-vllm_amd"))

import torch


def time_fn(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def build_cache(B, HKV, D, PS, L, dtype, dev, layers=1, seed=0):
    """`layers` independent caches so consecutive launches do not re-hit the 256 MiB Infinity Cache."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    P = -(-L // PS)
    n_pages = (B + 1) * HKV * P
    caches = []
    for _ in range(layers):
        kc = torch.randn(n_pages * PS, D, device=dev, dtype=dtype)
        vc = torch.randn(n_pages * PS, D, device=dev, dtype=dtype)
        caches.append((kc, vc))
    pt = torch.randperm(n_pages, generator=g).view(B + 1, HKV, P).to(torch.int32).to(dev)
    bm = torch.arange(1, B + 1, dtype=torch.int32, device=dev)
    lens = torch.full((B, HKV), L, dtype=torch.int32, device=dev)
    return caches, pt, bm, lens


def bench_decode(args):
    import compactor_vllm_amd.attention.sparse_decode_kernel as dk

    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    B, HQ, HKV, D, PS, L = args.B, 32, 8, 128, 128, args.L
    layers = max(1, min(32, int(600e6 // (2 * B * HKV * L * D * 2)) + 1))
    caches, pt, bm, lens = build_cache(B, HKV, D, PS, L, dtype, dev, layers)
    q = torch.randn(B, HQ, D, device=dev, dtype=dtype)
    splits_list = [args.splits] if args.splits else [16, 32, 64]
    bytes_alg = 2 * D * 2 * B * HKV * L + 2 * B * HQ * D * 2
    fp8 = args.kv_dtype == "fp8"
    if fp8:  # e4m3 codes + one fp32 scale per row (csrc/kv_fp8.hip); bytes = (2 D + 8) * sum L + 4 * B * HQ * D
        caches = [(kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)) for kc, vc in caches]
        scales = [(torch.rand(kc.shape[0], device=dev) * 0.01 + 0.005, torch.rand(kc.shape[0], device=dev) * 0.01 + 0.005)
                  for kc, _ in caches]
        bytes_alg = (2 * D + 8) * B * HKV * L + 4 * B * HQ * D
    elif args.kv_dtype == "mxfp4":  # random e2m1 codes + e8m0 scales around 2^-2 (csrc/kv_mxfp4.hip); bytes = (D + D/8) * sum L + ...
        rows = caches[0][0].shape[0]
        caches = [tuple(torch.randint(0, 256, (rows, D // 2), device=dev, dtype=torch.uint8) for _ in range(2))
                  for _ in caches]
        scales = [tuple(torch.randint(123, 128, (rows, D // 32), device=dev, dtype=torch.uint8) for _ in range(2))
                  for _ in caches]
        bytes_alg = (D + D // 8) * B * HKV * L + 4 * B * HQ * D
    else:
        scales = [(None, None)] * len(caches)
    from compactor_vllm_amd import _lib
    if args.flush:
        junk_a = torch.empty(128 << 20, dtype=torch.uint8, device=dev)
        junk_b = torch.empty_like(junk_a)
    for variant in [0]:
        for S in splits_list:
            dk.plan_internal_splits = lambda n_bh, bound, ks, S=S: S
            # one HIP graph with `layers` launches over distinct caches: no host launch overhead in the timing
            dk.head_sparse_decode_attention(q, caches[0][0], caches[0][1], lens, pt, bm, HKV, PS, k_scale=scales[0][0],
                                            v_scale=scales[0][1])
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for (kc, vc), (ksc, vsc) in zip(caches, scales):
                    if args.flush:  # stream 256 MB through the L2s between launches: the metadata lines go cold, as they
                        junk_b.copy_(junk_a)  # do between two layers of a decode step (the GEMVs' weights in between)
                    out = dk.head_sparse_decode_attention(q, kc, vc, lens, pt, bm, HKV, PS, k_scale=ksc, v_scale=vsc)
            us = time_fn(g.replay, iters=50, warmup=max(3, int(40e3 / (25.0 * layers)))) / layers  # ~40 ms of warm replays: settled clocks
            print(f"decode{'' if args.kv_dtype == 'model' else ' kv=' + args.kv_dtype} variant={variant} B={B} L={L} splits={S:3d} layers={layers}: {us:8.2f} us/(stage1+merge)  "
                  f"{bytes_alg / us / 1e6:7.3f} TB/s algorithmic", flush=True)


def bench_decode_step(args):
    """`decode --step`: the period of one whole decode-layer step (append the token's K/V row, attend, publish the
    lengths) under graph replay, `layers` steps over distinct caches per graph: the four-call sequence (index_select,
    decode_store_kv, attention, index_copy_) - timed twice, the difference is the run-to-run spread - and
    fused_decode_step.  `--lse`: both legs also return the LSE, i.e. the append rank's step of a split-KV decode (the
    four-call leg is what that rank ran before fused_decode_step had return_lse).  Splits as planned by default.  Every
    replay appends a row, so the caches have slack pages and every leg starts from the same lengths."""
    import compactor_vllm_amd.attention.sparse_decode_kernel as dk
    from compactor_vllm_amd.kv_cache.store_kv_cache import decode_store_kv

    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    B, HQ, HKV, D, PS, L = args.B, 32, 8, 128, 128, args.L
    slack = 4096  # rows a leg may append: warm replays + timed replays
    layers = max(1, min(32, int(600e6 // (2 * B * HKV * L * D * 2)) + 1))
    caches, pt, bm, _ = build_cache(B, HKV, D, PS, L + slack, dtype, dev, layers)
    fp8 = args.kv_dtype == "fp8"
    scales = [{}] * layers
    if fp8:
        caches = [(kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)) for kc, vc in caches]
        scales = [dict(k_scale=torch.rand(kc.shape[0], device=dev) * 0.01 + 0.005,
                       v_scale=torch.rand(kc.shape[0], device=dev) * 0.01 + 0.005) for kc, _ in caches]
    tables = [torch.zeros(B + 1, HKV, dtype=torch.int32, device=dev) for _ in range(layers)]
    bm_long = bm.long()
    qkv = torch.randn(B, HQ + 2 * HKV, D, device=dev, dtype=dtype)  # key / value: views of the fused projection
    q, k, v = qkv[:, :HQ].contiguous(), qkv[:, HQ:HQ + HKV], qkv[:, HQ + HKV:]

    def four_calls():
        for (kc, vc), sc, table in zip(caches, scales, tables):
            seq = table.index_select(0, bm)
            decode_store_kv(key=k, value=v, batch_mapping=bm, bh_lens=seq, page_table=pt, k_cache=kc, v_cache=vc,
                            PAGE_SIZE=PS, **sc)
            dk.head_sparse_decode_attention(q, kc, vc, seq, pt, bm, HKV, PS, return_lse=args.lse, **sc)
            table.index_copy_(0, bm_long, seq)

    def fused():
        for (kc, vc), sc, table in zip(caches, scales, tables):
            dk.fused_decode_step(q, k, v, kc, vc, table, pt, bm, HKV, PS, return_lse=args.lse, **sc)

    side = torch.cuda.Stream(dev)
    warm = max(3, int(40e3 / (25.0 * layers)))  # ~40 ms of warm replays: settled clocks
    iters = 200
    assert 1 + warm + iters <= slack
    us = {}
    for name, step in (("four-call", four_calls), ("fused", fused), ("four-call again", four_calls)):
        for table in tables:
            table.fill_(L)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # the per-stream workspace is allocated here, not inside the capture
            step()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            step()
        us[name] = time_fn(g.replay, iters=iters, warmup=warm) / layers
        assert int(tables[0][1, 0]) == L + 1 + warm + iters, "every replay must append one row"
        print(f"decode step kv={'fp8' if fp8 else 'bf16'} B={B} L={L} layers={layers} {name:15s}: {us[name]:8.2f} us/layer",
              flush=True)
    spread = abs(us["four-call"] - us["four-call again"])
    print(f"decode step kv={'fp8' if fp8 else 'bf16'} B={B} L={L}: fused - four-call = "
          f"{us['fused'] - min(us['four-call'], us['four-call again']):+.2f} us/layer, four-call spread {spread:.2f} us",
          flush=True)


def bench_prefill(args):
    from compactor_vllm_amd.attention.sparse_varlen_kernel import causal_sparse_varlen_with_cache

    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    B, HQ, HKV, D, PS = args.B, 32, 8, 128, 128
    for L in ([args.L] if args.L != 16384 or True else []):
        N = B * L
        q = torch.randn(N, HQ, D, device=dev, dtype=dtype)
        k = torch.randn(N, HKV, D, device=dev, dtype=dtype)
        v = torch.randn(N, HKV, D, device=dev, dtype=dtype)
        if args.fused_v:  # the engine's layout: V is a strided view of the fused projection output [N, (HQ + 2 HKV) D]
            qkv = torch.randn(N, (HQ + 2 * HKV) * D, device=dev, dtype=dtype)
            v = qkv[:, (HQ + HKV) * D:].view(N, HKV, D)
            if args.fused_v > 1:
                k = qkv[:, HQ * D:(HQ + HKV) * D].view(N, HKV, D)
        Pc = args.prefix  # cached prefix rows per head in front of the L appended tokens
        caches, pt, bm, lens = build_cache(B, HKV, D, PS, max(Pc, 1), dtype, dev)
        kc, vc = caches[0]
        lens.fill_(Pc)
        scales = {}
        if args.kv_dtype == "fp8":  # e4m3 codes + one fp32 scale per row: cvllm_prefill_attn_fp8 (csrc/prefill_fp8.hip)
            kc, vc = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
            scales = dict(k_scale=torch.rand(kc.shape[0], device=dev) * 0.01 + 0.005,
                          v_scale=torch.rand(kc.shape[0], device=dev) * 0.01 + 0.005)
        elif args.kv_dtype == "mxfp4":  # random e2m1 codes + e8m0 scales around 2^-2: cvllm_prefill_attn_mxfp4 when Pc > 0
            rows = kc.shape[0]
            kc, vc = (torch.randint(0, 256, (rows, D // 2), device=dev, dtype=torch.uint8) for _ in range(2))
            scales = {n: torch.randint(123, 128, (rows, D // 32), device=dev, dtype=torch.uint8)
                      for n in ("k_scale", "v_scale")}
        cu = torch.arange(0, B + 1, dtype=torch.int32, device=dev) * L
        fn = lambda: causal_sparse_varlen_with_cache(q, k, v, kc, vc, lens, pt, bm, cu, L, Pc, HKV, PS, **scales)
        # warm until ~40 ms of this kernel have run: with 2 warm launches a 16 K kernel (2 ms) was still timed on a ramping
        # clock (2.30 ms against 2.03 steady, profiles/r02_prefill_workgroup_stamps.txt)
        warm = max(2, min(40, int(40e-3 / (4e-9 * 2 * L * (L / 2 + Pc) * B / 1e3 + 1e-4))))
        us = time_fn(fn, iters=max(5, warm // 2), warmup=warm)
        flops = 4 * D * HQ * B * (L * Pc + L * (L + 1) / 2)
        print(f"prefill{' kv=' + args.kv_dtype if scales else ''} B={B} L={L} prefix={Pc}: {us / 1e3:9.3f} ms  "
              f"{flops / us / 1e6:8.1f} TFLOP/s (causal flops)", flush=True)


def bench_scoring(args):
    """Stand-alone cost of every store-stream / scoring kernel at the C3 layer shape (nothing else running)."""
    from compactor_vllm_amd.compression.common import extract_and_store_top_kv, select_retained
    from compactor_vllm_amd.compression.compactor import approximate_leverage_scores, non_causal_attn_scores
    from compactor_vllm_amd.compression.snapkv import query_aware_key_scores
    from compactor_vllm_amd.kv_cache.store_kv_cache import prefill_store_all_kv

    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    B, HQ, HKV, D, PS, L = args.B, 32, 8, 128, 128, args.L
    N = B * L
    q = (torch.randn(N, HQ, D, device=dev) * 0.3).to(dtype)
    k = (torch.randn(N, HKV, D, device=dev) * 0.3).to(dtype)
    v = torch.randn(N, HKV, D, device=dev).to(dtype)
    PHI = (torch.randn(D, 48, device=dev) / 48 ** 0.5).to(dtype)
    cu = (torch.arange(0, B + 1, device=dev) * L).to(torch.int32)
    lens = [L] * B
    P = -(-L // PS)
    n_pages = (B + 1) * HKV * P
    pt = torch.randperm(n_pages, device=dev).view(B + 1, HKV, P).to(torch.int32)
    bm = torch.arange(1, B + 1, dtype=torch.int32, device=dev)
    kc = torch.zeros(n_pages * PS, D, dtype=dtype, device=dev)
    vc = torch.zeros_like(kc)
    pre = approximate_leverage_scores(k, lens, PHI, normalize=True, chunk_size=512)
    sc = non_causal_attn_scores(q, k, v, cu, L, chunk_size=128, sm_scale=1.0, normalize=True, accum_scores=pre,
                                context_lens=lens, protected_first_tokens=[16] * B, protected_last_tokens=[64] * B,
                                accum_blending=0.5)
    retain = torch.tensor([max(int(round(0.5 * (L - 80) * HKV)), 1)] * B, dtype=torch.int32, device=dev)
    zero = torch.zeros(B, HKV, dtype=torch.int32, device=dev)

    def store_top():
        l = zero.clone()
        extract_and_store_top_kv(sc, cu, L, L * HKV, HKV, k, v, retain, pt, bm, l, kc, vc, PS)

    def store_all():
        l = zero.clone()
        prefill_store_all_kv(new_keys=k, new_values=v, cu_seqlens_k=cu, max_seqlen_k=L, k_cache=kc, v_cache=vc,
                             page_table=pt, bh_lens=l, batch_mapping=bm, PAGE_SIZE=PS)

    items = [
        ("leverage (sketch+solve+zscore)", lambda: approximate_leverage_scores(k, lens, PHI, normalize=True, chunk_size=512)),
        ("chunk mass + zscore + blend + protect", lambda: non_causal_attn_scores(
            q, k, v, cu, L, chunk_size=128, sm_scale=1.0, normalize=True, accum_scores=pre, context_lens=lens,
            protected_first_tokens=[16] * B, protected_last_tokens=[64] * B, accum_blending=0.5)),
        ("snapkv scores", lambda: query_aware_key_scores(q, k, cu, cu, w=32, max_seqlen_k=L)),
        ("select (joint + per-head)", lambda: select_retained(sc, cu, L, retain, bm, zero, PS, True)),
        ("select + compaction", store_top),
        ("store_all", store_all),
    ]
    if args.prefix > 0:
        # SnapKV on the last chunk of a chunked prefill: --L new tokens over --prefix cached rows per head
        from compactor_vllm_amd.compression.snapkv import query_aware_key_scores_paged
        assert B == 1, "--prefix: one sequence, as the chunked prefill runs it"
        Pc, fp8 = args.prefix, args.kv_dtype == "fp8"
        caches, ppt, pbm, _ = build_cache(B, HKV, D, PS, Pc, dtype, dev)
        pkc, pks = caches[0][0] * 0.3, None
        if fp8:
            pkc, pks = (pkc * 30).to(torch.float8_e4m3fn), torch.rand(pkc.shape[0], device=dev) * 0.01 + 0.005
        cu_all = torch.tensor([0, Pc + L], dtype=torch.int32, device=dev)

        def gather_plain():  # what the hook did before the paged kernel: torch gather (+ dequantise) + the plain kernel
            k_all = torch.empty((Pc + L, HKV, D), dtype=dtype, device=dev)
            pos = torch.arange(Pc, device=dev)
            rows = ppt[pbm[0].long()].long()[:, pos // PS] * PS + (pos % PS)[None, :]
            if fp8:
                codes = pkc.view(torch.uint8)[rows].view(torch.float8_e4m3fn)
                k_all[:Pc] = (codes.float() * pks[rows][..., None]).to(dtype).transpose(0, 1)
            else:
                k_all[:Pc] = pkc[rows].transpose(0, 1)
            k_all[Pc:] = k
            return query_aware_key_scores(q, k_all, cu, cu_all, w=32, max_seqlen_k=Pc + L)

        e, s_ = (1, 4) if fp8 else (2, 0)
        nbytes = 2 * HKV * (Pc * (D * e + s_) + L * D * 2)  # both passes read every key once
        tag = f"prefix={Pc} kv={'fp8' if fp8 else 'bf16'} ({nbytes / 1e6:.1f} MB algorithmic)"
        items += [(f"snapkv gather + plain, {tag}", gather_plain),
                  (f"snapkv paged, {tag}", lambda: query_aware_key_scores_paged(
                      q, k, cu, cu, cu_all, pkc, ppt, pbm, PS, 32, k_scale=pks, max_seqlen_k=Pc + L)),
                  (f"snapkv gather + plain (repeat), {tag}", gather_plain)]
    if args.with_producer:
        from compactor_vllm_amd.layers.rotary_embedding import fused_qkv_rope, get_rope
        rope = get_rope(D, D, max(L, 1024), 500000.0, None).to(dev)
        qkv = torch.randn(N, (HQ + 2 * HKV) * D, device=dev).to(dtype)
        pos = torch.arange(L, device=dev).repeat(B)
        items.append(("qkv split + rope producer", lambda: fused_qkv_rope(qkv, pos, rope.cos_sin_cache, HQ, HKV, D)))
    if args.only:
        items = [it for it in items if args.only in it[0]]
    for name, fn in items:
        # default ~30 ms of warm calls: settled clocks (3 warm calls read 5-15 % higher)
        us = time_fn(fn, iters=args.iters or 50, warmup=args.warmup if args.warmup >= 0 else 300)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        print(f"scoring B={B} L={L}: {name:42s} {us:9.1f} us  peak temporaries {peak / 2**20:8.1f} MiB", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what")
    ap.add_argument("--L", type=int, default=16384)
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--splits", type=int, default=0)
    ap.add_argument("--variant", type=int, default=-1)
    ap.add_argument("--fused-v", type=int, default=0, help="prefill: 1 = V (2 = K and V) as strided views of a fused qkv buffer")
    ap.add_argument("--kv-dtype", choices=["model", "fp8", "mxfp4"], default="model",
                    help="decode, prefill, scoring --prefix: the cache's element type - the model dtype (bf16) or FP8 e4m3 codes + per-row scales; "
                         "decode (not --step) and prefill only: mxfp4 = e2m1 codes + e8m0 block scales")
    ap.add_argument("--prefix", type=int, default=0, help="prefill, scoring (SnapKV items): cached prefix rows per head in front of the --L appended tokens")
    ap.add_argument("--step", action="store_true", help="decode: whole layer steps (append + attend + lengths), four-call against fused")
    ap.add_argument("--lse", action="store_true", help="decode --step: both legs also return the LSE (the split-KV append rank's step)")
    ap.add_argument("--flush", action="store_true", help="decode: a 128 MB device copy between launches (cold metadata, as inside a decode step)")
    ap.add_argument("--iters", type=int, default=0)      # scoring: timed calls per item (0 = default)
    ap.add_argument("--warmup", type=int, default=-1)    # scoring: warm calls per item (-1 = default)
    ap.add_argument("--with-producer", action="store_true")  # scoring: add the f-2 producer kernel
    ap.add_argument("--only", default="")                # scoring: substring filter on the item name
    a = ap.parse_args()
    if a.kv_dtype == "mxfp4" and (a.what == "scoring" or a.step):
        ap.error("--kv-dtype mxfp4: decode and prefill attention only (no fused step, no scoring reads)")
    {"decode": bench_decode_step if a.step else bench_decode, "prefill": bench_prefill, "scoring": bench_scoring}[a.what](a)
