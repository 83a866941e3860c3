"""FP8 K / V cache against the 16-bit cache at Mistral-7B widths, both in ONE process, the two alternating over the rounds (a drifting box hits both alike);
prints one JSON line:
  decode_attn_us    HIP-event time of the decode attention launch of a layer (profiling class SM_PROF_ATTN; the split merge launch is outside the bracket in both
                    modes) at 512 streams x 336 keys, 128 streams x 2048 keys (sm_group_llm_decode) and 1 stream x 4096 keys (sm_llm_decode)
  group512_ms_step  ms per batched decode step at 512 streams (host clock around 64 steps ending in a synchronise: ~0.8 s per window)
  prefill2048_tok_s tokens/s of a 2048-token prefill into an empty stream, 12 prefills per window (~0.35 s; the fp8 leg pays the quantising append and the
                    per-layer expansion)
  kv_bytes_stream   sm_stream_kv_bytes of a stream holding 336 tokens

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
            st.close()
    for name in legs:
        res[name]["decode_attn_us"]["1x4096"] = {"median": round(statistics.median(per[name]), 2), "runs": [round(v, 2) for v in per[name]]}
        for k in ("group512_ms_step", "prefill2048_tok_s"):
            res[name][k] = {"median": statistics.median(res[name][k]), "runs": res[name][k]}
    print(json.dumps({"kv_fp8_bench": res, "rounds": rounds}))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
