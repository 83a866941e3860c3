"""Device-side sampling (csrc/sample.hip) at Mistral-7B shapes: one JSON line.
    python tools/sample_bench.py [--no-model]

  kernel   us per call of sm_sample_rows (T 0.7, top_p 0.9, caller's uniforms) at V = 32 000 for 1 / 32 / 128 / 512 rows of N(0, 6^2) logits, next to the
           arg-max kernel of the same shape (torch.ops-free: sm_argmax for one row, the cross-entropy kernel's arg-max output -- one block per row -- beyond).
           The operator carries its rules by value, 32 rows per launch: 512 rows are 16 launches.
  reply    tokens/s of a 256-token sampled reply on one stream (328-token context): the host-side sampler of generate(do_sample=True) (one step, one
           sync, torch sort + softmax + cumsum + multinomial per token), the device path (decode_chunk 16 steps per sync) and the greedy loop
  group    tokens/s of a 32-stream group decode, all streams sampled against all greedy
Each timed window is warmed up with the same shapes, ends in a device synchronise and is repeated (median of 5)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from streammind_amd import _lib, native
from streammind_amd.model import Videollama2MistralForCausalLM
from streammind_amd.native import NativeModel, PathConfig

V = 32000


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def kernel_leg():
    lib = _lib.load()
    out = {"rows": [], "sample_us": [], "argmax_us": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    for M in (1, 32, 128, 512):
        lg = torch.randn(M, V, generator=g, device="cuda") * 6
        u = torch.rand(M, generator=g, device="cuda")
        am = torch.empty(M, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        n = 200

        def samp():
            for _ in range(n):
                native.sample_rows(lg, (0.7, 0.9, 0, 0), u=u)

        def amax():
            for _ in range(n):
                if M == 1:
                    lib.sm_argmax(lg.data_ptr(), V, am.data_ptr(), st)
                else:
                    lib.sm_cross_entropy(lg.data_ptr(), M, V, V, None, -100, None, am.data_ptr(), st)
        out["rows"].append(M)
        out["sample_us"].append(round(timed(samp) / n * 1e6, 2))
        out["argmax_us"].append(round(timed(amax) / n * 1e6, 2))
    return out


def reply_leg(model, cfg, n_ctx=328, n_new=256):
    m = Videollama2MistralForCausalLM(model, max_frames=8, max_seq=1024, eos_token_id=None)
    prompt = torch.randint(3, cfg.llm_vocab, (1, n_ctx), generator=torch.Generator().manual_seed(3))
    out = {"context_tokens": n_ctx, "new_tokens": n_new}
    for name, kw in (("greedy", dict(do_sample=False)), ("host_sampled", dict(do_sample=True, temperature=0.7, top_p=0.9)),
                     ("device_sampled", dict(do_sample=True, temperature=0.7, top_p=0.9, device_sampling=True, seed=11))):
        out[name + "_tokens_per_s"] = round(n_new / timed(lambda: m.generate(prompt, max_new_tokens=n_new, **kw), reps=3), 1)
    return out


def group_leg(model, cfg, S=32, n_ctx=328, n_new=48):
    g = torch.Generator(device="cuda").manual_seed(17)
    streams = []
    for _ in range(S):
        st = model.open_stream(max_frames=8, max_seq=1024)
        st.prefill(torch.randint(3, cfg.llm_vocab, (n_ctx,), generator=g, device="cuda", dtype=torch.int32))
        streams.append(st)
    grp = model.open_group(streams)
    out = {"streams": S, "context_tokens": n_ctx}

    def run():
        for st in streams:
            st.set_kv_len(n_ctx)
        grp.decode(n_new)
    for name, rule in (("greedy", None), ("sampled", (0.7, 0.9, 0))):
        for i, st in enumerate(streams):
            st.set_sampling(None) if rule is None else st.set_sampling(*rule, seed=i)
        out[name + "_tokens_per_s"] = round(S * n_new / timed(run), 1)
    return out


if __name__ == "__main__":
    res = {"kernel": kernel_leg()}
    if "--no-model" not in sys.argv:
        cfg = PathConfig(llm_layers=32, max_frames_per_call=1, vit_layers=2)
        model = NativeModel(cfg)
        bench.random_weights_into(model, cfg, 1)
        bench.random_llm_weights_into(model, cfg, 2)
        model.finalize()
        res["reply"] = reply_leg(model, cfg)
        res["group"] = group_leg(model, cfg)
    print(json.dumps(res))
