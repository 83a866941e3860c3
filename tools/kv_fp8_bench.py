"""FP8 K / V cache against the 16-bit cache at Mistral-7B widths, both in ONE process, the two alternating over the rounds (a drifting box hits both alike);
prints one JSON line:
  decode_attn_us    HIP-event time of the decode attention launch of a layer (profiling class SM_PROF_ATTN; the split merge launch is outside the bracket in both
                    modes) at 512 streams x 336 keys, 128 streams x 2048 keys (sm_group_llm_decode) and 1 stream x 4096 keys (sm_llm_decode)
  group512_ms_step  ms per batched decode step at 512 streams (host clock around 64 steps ending in a synchronise: ~0.8 s per window)
  prefill2048_tok_s tokens/s of a 2048-token prefill into an empty stream, 12 prefills per window (~0.35 s; the fp8 leg pays the quantising append and the
                    per-layer expansion)
  kv_bytes_stream   sm_stream_kv_bytes of a stream holding 336 tokens
  chunk_attn_us     (fp8 cache only) HIP-event time of one layer's chunk attention work at H = 32, KV = 8, capacity 4096, per (n, pos0): `expand_bf16` = what
                    llm_layers issues with kv_fp8_chunk off (sm_kv_fp8_expand over the visible keys + the 16-bit chunk kernel), `expand_only` = that expansion
                    alone, `fused` = with the switch on (sm_llm_attention_fp8 incl. its split merge); 200 calls per bracket (50 from 512 rows), the three alternating over the rounds
  prefill2048_tok_s_chunk  the fp8 leg's 2048-token prefill with kv_fp8_chunk on

    python tools/kv_fp8_bench.py [rounds]"""
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


def attn_us(m, run, steps):
    """us per decode-attention launch over `steps` decode steps issued by run(steps)"""
    run(2); torch.cuda.synchronize()
    m.lib.sm_prof_reset(); m.lib.sm_prof_enable(1 << 2)
    run(steps); torch.cuda.synchronize()
    m.lib.sm_prof_enable(0)
    cnt, ms = C.c_int(), C.c_float()
    m.lib.sm_prof_read(2, C.byref(cnt), C.byref(ms))
    return ms.value * 1e3 / max(cnt.value, 1)


CHUNK_POINTS = ((16, 4080), (64, 4032), (512, 1536), (2048, 0))


def chunk_attn_us(lib, rounds):
    H, KV, cap, nc = 32, 8, 4096, 4096 * 8 * 128
    g = torch.Generator(device="cuda").manual_seed(3)
    kb, vb = (torch.randint(0, 0x78, (cap * KV * 132,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2))      # finite codes, scales 2^-6
    for b in (kb, vb):
        b[nc:].view(torch.float32).fill_(2.0 ** -6)
    q = torch.randn(2048, H * 128, device="cuda", generator=g).bfloat16()
    ctx, kx, vx, ws = torch.empty_like(q), torch.zeros(nc, dtype=torch.bfloat16, device="cuda"), torch.zeros(nc, dtype=torch.bfloat16, device="cuda"), torch.empty(16 * 32 * H * 130, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())

    def legs(n, pos0):
        expand = lambda: lib.sm_kv_fp8_expand(P(kb), P(vb), 0, pos0 + n, KV, 128, cap, P(kx), P(vx), st)
        return {"expand_bf16": lambda: expand() or lib.sm_llm_attention(P(q), P(kx), P(vx), n, pos0, H, KV, 128, cap, P(ctx), st), "expand_only": expand,
                "fused": lambda: lib.sm_llm_attention_fp8(P(q), P(kb), P(vb), n, pos0, H, KV, 128, cap, 0, P(ws), ws.numel(), P(ctx), st)}

    out = {}
    for n, pos0 in CHUNK_POINTS:
        per, iters = {name: [] for name in legs(n, pos0)}, (200 if n <= 64 else 50)          # windows of 10 ms and more
        for _ in range(rounds):
            for name, fn in legs(n, pos0).items():
                assert fn() == 0
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record(); torch.cuda.synchronize()
                per[name].append(round(e0.elapsed_time(e1) * 1e3 / iters, 2))
        out[f"{n}@{pos0}"] = {name: {"median": statistics.median(v), "runs": v} for name, v in per.items()}
    return out


def main(rounds=3):
    legs = {"bf16": make_model(), "fp8": make_model(kv_fp8=True)}
    g = torch.Generator(device="cuda").manual_seed(17)
    ids = lambda n: torch.randint(3, 32000, (n,), generator=g, device="cuda", dtype=torch.int32)
    res = {name: {"decode_attn_us": {}, "group512_ms_step": [], "prefill2048_tok_s": []} for name in legs}
    for S, ctx, key in ((512, 336, "512x336"), (128, 2048, "128x2048")):
        groups = {}
        for name, (cfg, m) in legs.items():
            streams = [m.open_stream(max_frames=8, max_seq=4096) for _ in range(S)]
            for st in streams:
                st.prefill(ids(ctx - 12))
            if S == 512:
                res[name]["kv_bytes_stream"] = streams[0].kv_bytes()
            groups[name] = (m.open_group(streams), streams)
        per = {name: [] for name in legs}
        for _ in range(rounds):
            for name, (cfg, m) in legs.items():
                grp, streams = groups[name]
                for st in streams:
                    st.set_kv_len(ctx - 12)
                per[name].append(attn_us(m, grp.decode, 8))           # contexts ctx - 10 .. ctx - 2 during the timed steps
                if S == 512:
                    for st in streams:
                        st.set_kv_len(ctx - 12)
                    grp.decode(4); torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    grp.decode(64); torch.cuda.synchronize()
                    res[name]["group512_ms_step"].append(round((time.perf_counter() - t0) / 64 * 1e3, 3))
        for name in legs:
            res[name]["decode_attn_us"][key] = {"median": round(statistics.median(per[name]), 2), "runs": [round(v, 2) for v in per[name]]}
            grp, streams = groups[name]
            grp.close()
            for st in streams:
                st.close()
    solo = {name: m.open_stream(max_frames=8, max_seq=4608) for name, (cfg, m) in legs.items()}
    for name, st in solo.items():
        st.prefill(ids(2048)); st.prefill(ids(2036))
    per = {name: [] for name in legs}
    for _ in range(rounds):
        for name, (cfg, m) in legs.items():
            solo[name].set_kv_len(4084)
            per[name].append(attn_us(m, solo[name].decode, 8))
            st = m.open_stream(max_frames=8, max_seq=2048)
            p = ids(2048)
            st.prefill(p); st.set_kv_len(0); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(12):
                st.prefill(p); st.set_kv_len(0)
            torch.cuda.synchronize()
            res[name]["prefill2048_tok_s"].append(round(12 * 2048 / (time.perf_counter() - t0), 1))
            if name == "fp8":                            # the same prefill with the fused chunk attention (the switch may be thrown at any time)
                assert m.lib.sm_model_set_kv_fp8_chunk(m.h, 1) == 0
                st.prefill(p); st.set_kv_len(0); torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(12):
                    st.prefill(p); st.set_kv_len(0)
                torch.cuda.synchronize()
                res[name].setdefault("prefill2048_tok_s_chunk", []).append(round(12 * 2048 / (time.perf_counter() - t0), 1))
                assert m.lib.sm_model_set_kv_fp8_chunk(m.h, 0) == 0
            st.close()
    for name in legs:
        res[name]["decode_attn_us"]["1x4096"] = {"median": round(statistics.median(per[name]), 2), "runs": [round(v, 2) for v in per[name]]}
        for k in ("group512_ms_step", "prefill2048_tok_s", "prefill2048_tok_s_chunk"):
            if k in res[name]:
                res[name][k] = {"median": statistics.median(res[name][k]), "runs": res[name][k]}
    res["fp8"]["chunk_attn_us"] = chunk_attn_us(legs["fp8"][1].lib, rounds)
    print(json.dumps({"kv_fp8_bench": res, "rounds": rounds}))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
