"""Mistral-7B decode-only micro-benchmark (for rocprofv3 kernel traces of the decode step).
--fp4 [n_new]: batch-1 decode on bf16, fp8 and MXFP4 weights in ONE run on one box, the formats alternating over three rounds: tokens/s (median), the
fraction of the HBM roof on each format's own bytes per token, the summed HIP-event time of the weight-streaming launches per token, the same per
product shape (us per launch, TB/s on the product's own weight bytes), and ms per batched decode step at 4 / 8 / 16 streams; then the wide groups.
--fp4-groups: only the wide groups -- batched decode at 32 / 64 / 128 streams on bf16, fp8 (32, 64: its cap) and MXFP4 mode 2 (weights_fp4=2: the fp4
weight stream of 17..128 rows), the formats alternating over three rounds (median ms per step), and for fp4 the HIP-event time of every product of a
layer (us per launch incl. its slab sum, TB/s on the product's own 4.25-bit bytes) and of the activation prepass launches (their share of a step).
--fp4-prefill: prefills of 328 and 2048 tokens on bf16, MXFP4 mode 2 (the per-call expansion above 128 rows) and mode 2 + fp4_gemm (the tiled fp4 GEMM),
the three alternating over three rounds in one process (median ms per prefill, min..max), and per product of a layer the HIP-event us per launch
(expansion leg: the product and, apart, the expansion launches in front of it; fp4_gemm leg: the product incl. its slab sum, and the prepass launches)."""
import ctypes as C
import json, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from streammind_amd.native import NativeModel, PathConfig


def make_model(**kw):
    cfg = PathConfig(llm_layers=32, max_frames_per_call=1, vit_layers=2, **kw)
    m = NativeModel(cfg)
    bench.random_weights_into(m, cfg, 1)
    bench.random_llm_weights_into(m, cfg, 2)
    m.finalize()
    return cfg, m


def wide_groups(rounds=3):
    legs = {name: make_model(**kw) for name, kw in (("bf16", {}), ("fp8", dict(weights_fp8=1)), ("fp4", dict(weights_fp4=2)))}
    sizes = {"bf16": (32, 64, 128), "fp8": (32, 64), "fp4": (32, 64, 128)}
    ms = {name: {S: [] for S in sizes[name]} for name in legs}
    for _ in range(rounds):                                                     # alternate: a drifting box hits every format alike
        for name, (cfg, m) in legs.items():
            grp = bench.group_decode_leg(m, cfg, sizes=sizes[name], n_new=32)
            for S, t in zip(grp["streams"], grp["ms_per_step"]):
                ms[name][S].append(t)
    out = {name: {S: {"ms_per_step": statistics.median(v), "runs": v} for S, v in per.items()} for name, per in ms.items()}
    cfg, m = legs["fp4"]                                                        # fp4: HIP events around every weight-streaming launch of 8 steps
    g = torch.Generator(device="cuda").manual_seed(17)
    streams = []
    for S in sizes["fp4"]:
        while len(streams) < S:
            st = m.open_stream(max_frames=8, max_seq=1024)
            st.prefill(torch.randint(3, cfg.llm_vocab, (328,), generator=g, device="cuda", dtype=torch.int32))
            streams.append(st)
        grp = m.open_group(streams)
        grp.decode(4); torch.cuda.synchronize()
        m.lib.sm_prof_reset(); m.lib.sm_prof_enable(1 << 1)
        grp.decode(8); torch.cuda.synchronize()
        m.lib.sm_prof_enable(0)
        grp.close()
        per, bpw = {}, 0.5 + 1 / 32
        for label, tag, byts in (("qkv", (6144 << 32) | 4096, 6144 * 4096 * bpw), ("o", (4096 << 32) | 4096, 4096 * 4096 * bpw), ("gate_up", (14336 << 32) | 4096, 2 * 14336 * 4096 * bpw),
                                 ("down", (4096 << 32) | 14336, 4096 * 14336 * bpw), ("prepass_k4096", (1 << 62) | 4096, 0), ("prepass_k14336", (1 << 62) | 14336, 0)):
            c2, m2 = C.c_int(), C.c_float()
            m.lib.sm_prof_read_tag(1, C.c_longlong(tag), C.byref(c2), C.byref(m2))
            if c2.value:
                us = m2.value * 1e3 / c2.value
                per[label] = {"launches_per_step": c2.value // 8, "us": round(us, 2), "ms_per_step": round(m2.value / 8, 4)}
                if byts:
                    per[label]["tb_s"] = round(byts / us / 1e6, 2)
        out["fp4"][S]["per_product"] = per
    print(json.dumps({"group_decode_wide": out}))


def three_formats(n_new):
    d, legs = 4096, {}
    for name, kw in (("bf16", {}), ("fp8", dict(weights_fp8=1)), ("fp4", dict(weights_fp4=True))):
        cfg, m = make_model(**kw)
        legs[name] = (cfg, m, m.open_stream(max_frames=1024, max_seq=1024))
    lin = 32 * (d * d * 2 + 2 * d * 1024 + 3 * d * 14336)                      # weights of the LLM's linears
    wbytes = {"bf16": 2.0 * lin, "fp8": 1.0 * lin + 4 * 32 * (6144 + 4096 + 28672 + 4096), "fp4": lin * (0.5 + 1 / 32)}
    tps = {k: [] for k in legs}
    for _ in range(3):                                                          # alternate: a drifting box hits every format alike
        for name, (cfg, m, s) in legs.items():
            tps[name].append(bench.decode_leg(m, s, cfg, n_new=n_new)["tokens_per_s"])
    out = {}
    for name, (cfg, m, s) in legs.items():
        t = statistics.median(tps[name])
        r = bench.decode_leg(m, s, cfg, n_new=16)["roofline"]
        rest = r["bytes_per_token"] - 2.0 * lin                                 # lm_head (bf16 in every format) + the K / V caches
        byts = wbytes[name] + rest
        lib = m.lib
        lib.sm_prof_reset(); lib.sm_prof_enable(1 << 1)                         # class 1: the weight-streaming launches
        s.decode(32); torch.cuda.synchronize()
        lib.sm_prof_enable(0)
        cnt, ms = C.c_int(), C.c_float()
        lib.sm_prof_read(1, C.byref(cnt), C.byref(ms))
        shapes = {}                                                             # per product of a layer: HIP-event us per launch, and TB/s on its own weight bytes
        bpw = {"bf16": 2.0, "fp8": 1.0, "fp4": 0.5 + 1 / 32}[name]
        for label, N, K, mats in (("qkv", 6144, 4096, 1), ("o", 4096, 4096, 1), ("gate_up", 14336, 4096, 2), ("down", 4096, 14336, 1), ("lm_head", cfg.llm_vocab, 4096, 1)):
            c2, m2 = C.c_int(), C.c_float()
            lib.sm_prof_read_tag(1, C.c_longlong((N << 32) | K), C.byref(c2), C.byref(m2))
            if c2.value:
                us = m2.value * 1e3 / c2.value
                shapes[label] = {"launches": c2.value, "us": round(us, 2), "tb_s": round(mats * N * K * (bpw if label != "lm_head" or name == "fp8" else 2.0) / us / 1e6, 2)}
        grp = bench.group_decode_leg(m, cfg, sizes=(4, 8, 16), n_new=48)       # batched decode, up to the 16 rows one fp4 weight pass takes
        shapes["group_decode_ms_per_step"] = dict(zip(grp["streams"], grp["ms_per_step"]))
        out[name] = {"per_shape": shapes, "tokens_per_s": round(t, 1), "runs": tps[name], "bytes_per_token": byts, "hbm_frac": round(byts * t / 1e9 / bench.HBM_PEAK_GBS, 4),
                     "weight_stream_ms_per_token": round(ms.value / 32, 4), "weight_stream_launches_per_token": cnt.value // 32, "ms_per_token": round(1e3 / t, 4)}
    print(json.dumps({"decode_three_formats": out}))
    del legs, out, m, s, cfg, grp                                               # (the streams hold their models: drop every name before the next three are built)
    import gc
    gc.collect(); torch.cuda.empty_cache()
    wide_groups()


def fp4_prefill(rounds=3, lengths=(328, 2048)):
    legs = {name: make_model(**kw) for name, kw in (("bf16", {}), ("fp4_expand", dict(weights_fp4=2)), ("fp4_gemm", dict(weights_fp4=2, fp4_gemm=True)))}
    g = torch.Generator(device="cuda").manual_seed(17)
    ids = {n: torch.randint(3, 32000, (n,), generator=g, device="cuda", dtype=torch.int32) for n in lengths}
    streams = {name: m.open_stream(max_frames=8, max_seq=max(lengths)) for name, (cfg, m) in legs.items()}

    def run(name, n, reps):
        st = streams[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            st.set_kv_len(0); st.prefill(ids[n])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    for name in legs:                                                           # every shape warmed before it is timed
        for n in lengths:
            run(name, n, 2)
    ms = {name: {n: [] for n in lengths} for name in legs}
    for _ in range(rounds):                                                     # alternate: a drifting box hits every leg alike
        for name in legs:
            for n in lengths:
                ms[name][n].append(run(name, n, 8 if n <= 512 else 3))
    out = {name: {n: {"ms_per_prefill": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for n, v in per.items()} for name, per in ms.items()}
    products = (("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336))
    for name, (cfg, m) in legs.items():                                         # HIP events around every product launch of two prefills (class 0: the tiled products)
        for n in lengths:
            m.lib.sm_prof_reset(); m.lib.sm_prof_enable(1 << 0)
            run(name, n, 2)
            m.lib.sm_prof_enable(0)

            def read(tag):
                c2, m2 = C.c_int(), C.c_float()
                m.lib.sm_prof_read_tag(0, C.c_longlong(tag), C.byref(c2), C.byref(m2))
                return (c2.value, round(m2.value * 1e3 / c2.value, 2)) if c2.value else (0, None)
            per = {}
            for label, N, K in products:
                cnt, us = read((N << 32) | K)
                if not cnt and label == "gate_up":                              # (the tiled fp4 GEMM runs gate | up in its w / w2 form: N = 14336)
                    cnt, us = read(((N // 2) << 32) | K)
                per[label] = {"launches": cnt, "us": us}
                ecnt, eus = read((1 << 61) | (N << 32) | K)
                if ecnt:
                    per[label]["expansion_us"] = eus
            for K in (4096, 14336):
                cnt, us = read((1 << 62) | K)
                if cnt:
                    per["prepass_k%d" % K] = {"launches": cnt, "us": us}
            out[name][n]["per_product"] = per
    print(json.dumps({"fp4_prefill": out}))


if "--fp4-prefill" in sys.argv:                                                 # [lengths, comma-separated: a scan for the dispatch's row bound]
    i = sys.argv.index("--fp4-prefill")
    fp4_prefill(lengths=tuple(int(v) for v in sys.argv[i + 1].split(",")) if len(sys.argv) > i + 1 else (328, 2048))
    sys.exit(0)
if "--fp4-groups" in sys.argv:
    wide_groups()
    sys.exit(0)
if "--fp4" in sys.argv:
    i = sys.argv.index("--fp4")
    three_formats(int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 128)
    sys.exit(0)

cfg = PathConfig(llm_layers=32, max_frames_per_call=1, vit_layers=2, weights_fp8=os.environ.get("FP8", "0") == "1", llm_fp16=os.environ.get("FP16", "0") == "1")    # short ViT: perception is not measured here; FP8=1: weight-only fp8 mode; FP16=1: fp16 operands (llm_fp16)
model = NativeModel(cfg)
bench.random_weights_into(model, cfg, 1)
bench.random_llm_weights_into(model, cfg, 2)
model.finalize()
s = model.open_stream(max_frames=16384, max_seq=int(sys.argv[2]) if len(sys.argv) > 2 else 1024)
nctx = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [256]        # frame tokens of the context (+ 72 text tokens)
for n in nctx:
    r = bench.decode_leg(model, s, cfg, n_ctx_frames=n, n_new=int(sys.argv[1]) if len(sys.argv) > 1 else 64)
    print(r if len(nctx) == 1 else {k: r[k] for k in ("context_tokens", "tokens_per_s", "ms_per_token")})
