"""Device-side temperature / top-k / top-p sampling (csrc/sample.hip) against an fp64 numpy statement of the rule in
include/streammind_hip.h, through the operator, the stream, the stream group and generate().

delta = 1e-5 of the row's mass: fp32 exp and the /T rounding move a term by ~|x| 2^-24 relative (below 3e-6 over a row), sums of 2^15 terms
add ~1e-6; delta is ~3x that and a third of the smallest mass that matters at V = 32 000 (1 / V = 3.1e-5)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DELTA = 1e-5
PARAMS = [(0.7, 0.9, 0), (0.2, 0.7, 0), (1.0, 0.95, 50), (1.0, 1.0, 0), (1.0, 1.0, 1)]          # (temperature, top_p, top_k)


def philox_u(seed, pos):
    """Philox4x32-10: key = (seed low, seed high), counter = (pos low, pos high, 0, 0); u = (out[0] >> 8) * 2^-24"""
    M = 0xFFFFFFFF
    c, k = [pos & M, (pos >> 32) & M, 0, 0], [seed & M, (seed >> 32) & M]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M, (p0 >> 32) ^ c[3] ^ k[1], p0 & M]
        k = [(k[0] + 0x9E3779B9) & M, (k[1] + 0xBB67AE85) & M]
    return np.float32((c[0] >> 8) * 2.0 ** -24), c


def ref_stats(l32, T):
    """fp64, from the same fp32 logits: p, above (mass of strictly greater logits), rank (number of them)"""
    l = l32.astype(np.float64)
    e = np.exp((l - l.max()) / np.float64(np.float32(T)))
    p = e / e.sum()
    order = np.argsort(-l, kind="stable")
    first = np.searchsorted(-l[order], -l[order], side="left")            # first member of each group of equal logits
    cs = np.concatenate([[0.0], np.cumsum(p[order])])
    above, rank = np.empty_like(p), np.empty(len(p), dtype=np.int64)
    above[order], rank[order] = cs[first], first
    return p, above, rank


def ref_keep(above, rank, top_p, top_k):
    return ((rank < top_k) if top_k > 0 else np.ones(len(rank), bool)) & ((above < top_p) if np.float32(top_p) < 1 else True)


def ref_token(p, keep, u):
    """-> (token, F_lo, F_hi per token): first id whose inclusive kept-CDF exceeds u * Z"""
    q = np.where(keep, p, 0.0)
    F = np.cumsum(q) / q.sum()
    hit = np.nonzero((F > np.float64(u)) & (q > 0))[0]
    return int(hit[0]) if len(hit) else int(np.nonzero(q > 0)[0][-1]), F - q / q.sum(), F


def check_row(l32, T, top_p, top_k, u, tok, kept):
    """the three conditions every row meets; -> (clear?, reference token)"""
    p, above, rank = ref_stats(l32, T)
    tp = np.float64(np.float32(top_p))
    keep = ref_keep(above, rank, tp, top_k)
    t_ref, Flo, Fhi = ref_token(p, keep, u)
    print(f"V={len(l32)} {T} {top_p} {top_k} u={u:.8f} tok={tok} ref={t_ref} kept={kept} ref_kept={int(keep.sum())} above={above[tok]:.3e} F=[{Flo[tok]:.8f},{Fhi[tok]:.8f}]")
    assert keep[tok] or abs(above[tok] - tp) <= DELTA
    assert Flo[tok] - DELTA <= u <= Fhi[tok] + DELTA
    if tp < 1:
        assert ref_keep(above, rank, tp - DELTA, top_k).sum() <= kept <= ref_keep(above, rank, tp + DELTA, top_k).sum()
    else:
        assert kept == keep.sum()
    clear = u - Flo[t_ref] > DELTA and Fhi[t_ref] - u > DELTA and (tp >= 1 or np.abs(above - tp).min() > DELTA)
    return clear, t_ref


@functools.lru_cache(maxsize=None)
def make_rows(V, M, ld, sigma):
    rng = np.random.default_rng(V * 131 + M)
    lg = np.full((M, ld), np.nan, dtype=np.float32)                         # the padding must never be read
    lg[:, :V] = (rng.standard_normal((M, V)) * sigma).astype(np.float32)
    if V > 2:
        lg[0, V // 3] = lg[0, 2 * V // 3] = lg[0, :V].max() + np.float32(0.5)     # two exactly equal logits at the top
        lg[M - 1, V // 2] = -np.inf
    u = rng.random(M).astype(np.float32)
    u[0] = 0.0
    if M > 1:
        u[1] = np.nextafter(np.float32(1), np.float32(0))
    return lg, u


# V = 40003 lies above the LDS-resident limit (160 KB per block less the histograms: ~34 600 columns): the variant that re-reads the row
@pytest.mark.parametrize("sigma", [6.0, 1.0])
@pytest.mark.parametrize("T,top_p,top_k", PARAMS)
@pytest.mark.parametrize("V,M,ld", [(1, 3, 1), (63, 33, 70), (1025, 3, 1025), (32000, 33, 32000), (32003, 1, 32003), (40003, 3, 40003)])
def test_operator_against_fp64_reference(V, M, ld, T, top_p, top_k, sigma):
    from streammind_amd.native import sample_rows
    lg, u = make_rows(V, M, ld, sigma)
    tok, kept, mass = sample_rows(torch.from_numpy(lg).cuda()[:, :V], (T, top_p, top_k, 0), u=torch.from_numpy(u).cuda(), return_kept=True)
    tok, kept = tok.cpu().numpy(), kept.cpu().numpy()
    for m in range(M):
        clear, t_ref = check_row(lg[m, :V], T, top_p, top_k, u[m], int(tok[m]), int(kept[m]))
        if clear:
            assert tok[m] == t_ref, (m, tok[m], t_ref)
        if top_k == 1:
            assert tok[m] == int(np.argmax(lg[m, :V]))


@pytest.mark.parametrize("T,top_p", [(0.7, 0.9), (0.2, 0.7)])
def test_operator_exact_on_clear_rows(T, top_p):
    """N(0, 6^2) logits at Mistral's width: at least 90 % of 64 seeded rows are clear for the reference, and every clear row's id is exact"""
    from streammind_amd.native import sample_rows
    rng = np.random.default_rng(7)
    lg = (rng.standard_normal((64, 32000)) * 6).astype(np.float32)
    u = rng.random(64).astype(np.float32)
    tok, kept, _ = sample_rows(torch.from_numpy(lg).cuda(), (T, top_p, 0, 0), u=torch.from_numpy(u).cuda(), return_kept=True)
    res = [check_row(lg[m], T, top_p, 0, u[m], int(tok[m]), int(kept[m])) for m in range(64)]
    assert sum(c for c, _ in res) >= 58
    assert all(int(tok[m]) == t for m, (c, t) in enumerate(res) if c)


def test_device_rng_is_philox():
    from streammind_amd.native import sample_rows
    assert [f"{w:08x}" for w in philox_u(0, 0)[1]] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]       # the published known answer
    rng = np.random.default_rng(3)
    lg = torch.from_numpy((rng.standard_normal((6, 1025)) * 2).astype(np.float32)).cuda()
    seeds = [0, 1, 0xDEADBEEF, 0x0123456789ABCDEF, 2 ** 64 - 1, 77]
    pos = [0, 5, 2 ** 32 + 3, 2 ** 40, 123456, 2 ** 32 - 1]
    params = [(1.0, 0.95, 0, s) for s in seeds]
    a = sample_rows(lg, params, pos=pos).cpu().tolist()
    u = torch.tensor([float(philox_u(s, p)[0]) for s, p in zip(seeds, pos)], dtype=torch.float32).cuda()
    assert a == sample_rows(lg, params, u=u).cpu().tolist()
    assert a == sample_rows(lg, params, pos=pos).cpu().tolist()


@pytest.fixture(scope="module")
def tiny():
    from oracle import streammind_oracle as O
    from oracle.make_golden import TINY_V as TV, TINY_C as TC, TINY_G as TG, TINY_L as TL
    from tests.util_models import build_native, conn_gate_weights
    return build_native(TV, TC, TG, O.make_vit_weights(TV, 41), conn_gate_weights(TC, TG, 86), TL, O.make_lm_weights(TL, 44), max_frames_per_call=6), TL.vocab


def replay(s, rule):
    """the operator on the stream's own logits, at the index the pending token will occupy, gives the pending token"""
    from streammind_amd.native import sample_rows
    lg, nt = s.logits()
    assert sample_rows(lg[None], rule, pos=[s.kv_len]).cpu().tolist() == nt.cpu().tolist()


def test_stream_path(tiny):
    m, vocab = tiny
    ctx = torch.randint(3, vocab, (21,), generator=torch.Generator().manual_seed(5), dtype=torch.int32).cuda()
    rule = (0.9, 0.95, 40, 0x1234567890)
    def run(rule, steps, cleared=False):
        s = m.open_stream(max_frames=8, max_seq=128)
        if rule:
            s.set_sampling(*rule)
        if cleared:
            s.set_sampling(None)
        s.prefill(ctx)
        ids = []
        for n in steps:
            if rule and not cleared:
                replay(s, rule)                                                 # (c): the operator on the stream's logits gives its pending token
            ids += s.decode(n).cpu().tolist()
        return ids
    greedy = run(None, [8])
    assert run(rule, [8], cleared=True) == greedy                               # (a)
    assert run(rule, [8]) == run(rule, [1] * 8)                                 # (b)
    assert run((1.0, 1.0, 1, 0), [3, 5]) == greedy                              # (d)


@pytest.mark.parametrize("S", [3, 33])
def test_group_path(tiny, S):
    m, vocab = tiny
    g = torch.Generator().manual_seed(S)
    ctxs = [torch.randint(3, vocab, (5 + 3 * (i % 7),), generator=g, dtype=torch.int32).cuda() for i in range(S)]
    rules = [None if i % 3 == 0 else (0.8, 0.9, 0, 1000 + i) for i in range(S)]
    ids = {}
    for mixed in (False, True):
        streams = [m.open_stream(max_frames=8, max_seq=128) for _ in range(S)]
        for s, c, r in zip(streams, ctxs, rules):
            if mixed and r:
                s.set_sampling(*r)
            s.prefill(c)
        grp = m.open_group(streams)
        out = []
        for _ in range(4):
            out.append(grp.decode(1).cpu()[:, 0].tolist())
            for s, r in zip(streams, rules):
                if mixed and r:
                    replay(s, r)
        ids[mixed] = out
        grp.close()
    for i in range(0, S, 3):                                                # the greedy streams: what an all-greedy group call gives
        assert [o[i] for o in ids[True]] == [o[i] for o in ids[False]]


def test_generate_device_sampling(tiny):
    from streammind_amd.model import Videollama2MistralForCausalLM
    from streammind_amd.native import sample_rows
    m, vocab = tiny
    prompt = torch.randint(3, vocab, (1, 17), generator=torch.Generator().manual_seed(9))

    def gen(chunk, seed, **kw):
        model = Videollama2MistralForCausalLM(m, max_frames=8, max_seq=128, eos_token_id=None)
        model.decode_chunk = chunk
        out = model.generate(prompt, do_sample=True, device_sampling=True, seed=seed, temperature=1.0, top_p=1.0, max_new_tokens=12, **kw)
        assert model.stream.get_sampling() is None                              # the rule is cleared at the end
        return out[0].tolist(), model.stream.kv_len
    # two seeds whose FIRST ids differ according to the reference (Philox + the fp64 rule on the prefill's logits), clear of every boundary
    s = m.open_stream(max_frames=8, max_seq=128)
    s.prefill(prompt[0].to(torch.int32).cuda())
    lg = s.logits()[0].cpu().numpy()
    p, above, rank = ref_stats(lg, 1.0)
    firsts = {}
    for seed in range(1, 9):
        u = philox_u(seed, 17)[0]
        t, Flo, Fhi = ref_token(p, ref_keep(above, rank, 1.0, 0), u)
        if u - Flo[t] > DELTA and Fhi[t] - u > DELTA:
            firsts.setdefault(t, seed)
    sa, sb = list(firsts.values())[:2]
    a1, kv = gen(1, sa)
    assert len(a1) == 12 and kv == 17 + 12 and a1[0] == [t for t, sd in firsts.items() if sd == sa][0]
    assert gen(8, sa)[0] == a1
    assert gen(8, sb)[0] != a1
    stopped, kv = gen(8, sa, stopping_criteria=[lambda ids, _: ids.shape[1] >= 3])
    assert stopped == a1[:3] and kv == 17 + 3
    with pytest.raises(ValueError):
        gen(8, sa, generator=torch.Generator())
