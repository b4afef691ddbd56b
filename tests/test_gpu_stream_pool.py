"""GPU: the streaming session pool end to end (engine.stream_pool; csrc/stream_pool.hip).  A session's logits and ids, concatenated over its calls, must equal those of
`engine.stream(1, C, Lmax)` fed the same pieces — torch.equal — whatever the other slots do, whichever slot it got and however many idle steps lie between its calls.
At head size 64 without a relative term the pool runs the per-slot chunk kernel where the lock-step step runs the full forward's kernel — a different summation
order —, so there it is held to the bf16-modelled oracle of the utterance alone (max < 0.03 / mean < 0.003), the bar of every bf16 forward path."""
import ctypes as C

import pytest
import torch

from helpers import seeded_state_dict, synth_feats
from huggingface_asr_amd import shapes
from test_gpu_stream import TINY_CAUSAL, _engine, _gap, _oracle_alone, run_stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CF = 4
W = 4 * CF


def run_pool(pool, sessions, dummies=0):
    """sessions: dicts(x (T, F), n frames, start = the step it opens at or after = the index of the session whose slot it waits for, idle = steps it sits out).  Whole
    chunks while more than one chunk is left, then the rest as the tail — run_stream's protocol.  dummies: sessions opened first and left idle for good.
    -> per session (logits cpu, ids, slot), per step {session: n_out}"""
    for _ in range(dummies):
        pool.open()
    st = [dict(s, pos=0, sid=None, done=False, logits=[], ids=[]) for s in sessions]
    trace, t = [], 0
    while not all(s["done"] for s in st):
        for s in st:
            if s["sid"] is None and not s["done"] and (s.get("start") == t or (s.get("after") is not None and st[s["after"]]["done"])):
                s["sid"] = pool.open()
        feed, finish, who = {}, {}, {}
        for i, s in enumerate(st):
            if s["sid"] is None or s["done"] or t in s.get("idle", ()):
                continue
            left = s["n"] - s["pos"]
            piece = s["x"][s["pos"]: s["pos"] + min(left, W)].to(DEV)
            (feed if left > W else finish)[s["sid"]] = piece
            who[s["sid"]] = i
        out = pool.step(feed, finish)
        assert set(out) == set(who)
        step = {}
        for sid, o in out.items():
            s = st[who[sid]]
            k = int(o["n_ids"])
            assert o["logits"].shape[0] == o["n_out"] == o["ids"].shape[0] and bool((o["ids"][k:] == -1).all())
            s["logits"].append(o["logits"].float().cpu())
            s["ids"] += o["ids"][:k].cpu().tolist()
            s["pos"] += W if sid in feed else s["n"] - s["pos"]
            s["done"] = o["final"]
            s["slot"] = sid
            step[who[sid]] = o["n_out"]
            assert o["final"] == (sid in finish) and (not o["final"] or o["total"] == (s["n"] + 3) // 4)
        trace.append(step)
        t += 1
        assert t < 1000
    torch.cuda.synchronize()
    return [(torch.cat(s["logits"], 0), s["ids"], s["slot"]) for s in st], trace


def alone(eng, x, n, Lmax):
    res, _ = run_stream(eng.stream(1, CF, Lmax), x[None], [n], check_plan=False)
    return res[0]


def check_equal(got, want, what):
    assert got[0].shape == want[0].shape, what
    assert torch.equal(got[0], want[0]), f"{what}: differs from the stream of one by {float((got[0] - want[0]).abs().max())}"
    assert got[1] == want[1], what


# ------------------------------------------------------------------ four utterances over three slots
LENGTHS = [143, 61, 250, 97]


@pytest.fixture(scope="module")
def four():
    sd = seeded_state_dict(TINY_CAUSAL, 44)
    x, _ = synth_feats(44, 4, 250, LENGTHS)
    eng = _engine(TINY_CAUSAL, sd)
    return dict(eng=eng, x=x, ref=[alone(eng, x[b], n, 64) for b, n in enumerate(LENGTHS)])


def schedule(x, order=(0, 1, 2, 3)):
    s = [dict(x=x[0], n=143, start=0, idle={2, 5, 6}), dict(x=x[1], n=61, start=0), dict(x=x[2], n=250, start=3), dict(x=x[3], n=97, after=1, idle={7})]
    s[3]["after"] = order.index(1)
    return [s[i] for i in order]


def test_sessions_equal_the_stream_of_one(four):
    got, trace = run_pool(four["eng"].stream_pool(3, CF, 64), schedule(four["x"]))
    assert [g[2] for g in got] == [0, 1, 2, 1]                           # the 97-frame session runs in the slot the 61-frame one freed
    for b in range(4):
        check_equal(got[b], four["ref"][b], f"session {b}")
    # the step in which the 61-frame session flushes while the two others feed: it emits its whole lookahead, they a chunk each
    assert [s for s in trace if s.get(1, 0) > CF] == [{0: 0, 1: 16, 2: 0}]


def test_one_slot_flushes_while_two_feed(four):
    """sessions 0 and 2 feed whole chunks in the step where session 1 takes its 13-frame tail: per layer its rows exceed theirs by up to L * r = 30, in one set of launches"""
    pool = four["eng"].stream_pool(3, CF, 64)
    sess = [dict(x=four["x"][0], n=143, start=0), dict(x=four["x"][1], n=61, start=0), dict(x=four["x"][2], n=250, start=0)]
    got, trace = run_pool(pool, sess)
    assert trace[3] == {0: 0, 1: 16, 2: 0}                                # 61 frames = 16 encoder frames, all emitted by the flush; the others still fill their lookahead
    for b in range(3):
        check_equal(got[b], four["ref"][b], f"session {b}")


def test_same_schedule_twice_and_other_slots(four):
    eng, x = four["eng"], four["x"]
    pool = eng.stream_pool(3, CF, 64)
    a, ta = run_pool(pool, schedule(x))
    b, tb = run_pool(pool, schedule(x))                                   # the same pool again: every slot is reused
    assert ta == tb
    c, _ = run_pool(eng.stream_pool(4, CF, 64), schedule(x, (1, 0, 2, 3)), dummies=1)       # a slot held by an idle session in front, the first two sessions swapped
    assert [g[2] for g in c] == [1, 2, 3, 1]
    order = (1, 0, 2, 3)
    for k in range(4):
        check_equal(b[k], a[k], f"second run, session {k}")
        check_equal(c[k], a[order[k]], f"other slots, session {order[k]}")


# ------------------------------------------------------------------ the other layer forms: one staggered three-session schedule each
VARIANTS = {"merge3": dict(merge_conv_kernel=3), "csgu_linear": dict(csgu_use_linear_after_conv=True, csgu_activation="gelu"),
            "rotary_nomacaron": dict(position_embeddings_type="rotary", use_macaron_ff=False),
            "rotary_hd64": dict(position_embeddings_type="rotary", hidden_size=128, num_attention_heads=2, intermediate_size=256),
            "nopos_hd64": dict(position_embeddings_type=None, hidden_size=128, num_attention_heads=2, intermediate_size=256)}
V_LENGTHS = [150, 83, 118]


def _variant(name):
    cfg = dict(TINY_CAUSAL, **VARIANTS[name])
    sd = seeded_state_dict(cfg, 43)
    x, _ = synth_feats(43, 3, 150, V_LENGTHS)
    sess = [dict(x=x[0], n=150, start=0, idle={4}), dict(x=x[1], n=83, start=1), dict(x=x[2], n=118, start=3, idle={5, 6})]
    return cfg, sd, x, sess, _engine(cfg, sd)


@pytest.mark.parametrize("name", ["merge3", "csgu_linear", "rotary_nomacaron"])
def test_variants_equal_the_stream_of_one(name):
    cfg, sd, x, sess, eng = _variant(name)
    got, _ = run_pool(eng.stream_pool(3, CF, 40), sess)
    for b, n in enumerate(V_LENGTHS):
        check_equal(got[b], alone(eng, x[b], n, 40), f"{name} session {b}")


@pytest.mark.parametrize("name", ["rotary_hd64", "nopos_hd64"])
def test_hd64_plain_attention_vs_oracle(name):
    """Head size 64 without a relative term: the per-slot chunk kernel with ref = 3, one launch per layer, against the oracle of each utterance alone.  Measured on
    MI355X over the six sessions: max 0.0088 .. 0.0138, mean 0.00220 .. 0.00248 (the stream of one, which runs the full forward's kernel, measures the same: at this
    size the two agree bit for bit, which the test prints and does not require)."""
    cfg, sd, x, sess, eng = _variant(name)
    got, _ = run_pool(eng.stream_pool(3, CF, 40), sess)
    for b, n in enumerate(V_LENGTHS):
        o = _gap(got[b][0].numpy(), _oracle_alone(sd, cfg, x[b], n))
        s1 = _gap(got[b][0].numpy(), alone(eng, x[b], n, 40)[0].numpy())
        msg = f"{name} session {b}: vs oracle max {o[0]:.4f} mean {o[1]:.5f}; vs stream(1) max {s1[0]:.4f} mean {s1[1]:.5f}"
        print(msg)
        assert o[0] < 0.03 and o[1] < 0.003, msg


# ------------------------------------------------------------------ refusals on the device side, the model surface
def test_step_refuses_bad_records(four):
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.streaming import pool_table
    eng = four["eng"]
    pool = eng.stream_pool(3, CF, 40)
    sid = pool.open()
    pool.step(feed={sid: four["x"][0, :W].to(DEV)})
    cs = pool._config()
    feats = torch.zeros((1, W, 80), device=DEV)
    table = torch.zeros((4096,), dtype=torch.int32, device=DEV)
    lbuf, ints = torch.zeros((64, cs.logits_ld), device=DEV), torch.zeros((3, 64), dtype=torch.int32, device=DEV)

    def rc(records):
        rec = torch.tensor(records, dtype=torch.int32)
        return _lib.lib().mi_ebf_stream_step_slots(C.byref(cs), eng._table, CF, 40, None if pool._pos is None else pool._pos.data_ptr(), pool._state.data_ptr(),
                                                   pool._state.numel(), feats.data_ptr(), rec.data_ptr(), len(records), table.data_ptr(), table.numel(), lbuf.data_ptr(),
                                                   ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), torch.cuda.current_stream().cuda_stream)

    good, _ = pool_table([(sid, 16, 16, False)], CF, 2, 15)
    bad = [list(good[0])]; bad[0][2], bad[0][3] = good[0][3], good[0][2]                       # frontiers that decrease
    assert rc(bad) == _lib.ERR_ARG
    far, _ = pool_table([(sid, 160, 16, False)], CF, 2, 15)                                    # 44 frames in a cache of 40
    assert rc(far) == _lib.ERR_ARG
    with pytest.raises(RuntimeError, match="max_frames"):
        pool.n_feat[sid] = 160
        pool.step(feed={sid: four["x"][0, :W].to(DEV)})
    torch.cuda.synchronize()


def test_model_pool_equals_engine_pool():
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.engine import cfg_from_hf
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    torch.manual_seed(0)
    model = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**dict(shapes.TINY, is_causal=True))).to(DEV).eval()
    x, _ = synth_feats(45, 2, 100, [100, 57])
    sess = [dict(x=x[0], n=100, start=0), dict(x=x[1], n=57, start=2)]
    a, _ = run_pool(model.stream_pool(2, CF, 32), sess)
    eng = _engine(cfg_from_hf(model.config), {k: v for k, v in model.state_dict().items()})
    b, _ = run_pool(eng.stream_pool(2, CF, 32), sess)
    for s in range(2):
        check_equal(a[s], b[s], f"session {s}")
