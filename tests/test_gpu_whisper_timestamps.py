"""GPU: Whisper timestamps -- ssak_dec_timestamp_step (ssak_amd/csrc/whisper_generate.hip), ``WhisperSeq2Seq.generate(timestamps=True)``
(ssak_amd/whisper_seq2seq.py), ``WhisperSeq2Seq.transcribe`` (ssak_amd/whisper_transcribe.py) and ``python -m ssak_amd.whisper_infer
--timestamps`` -- against the float64 restatement tests/whisper_timestamps_ref.py (held to transformers' WhisperTimeStampLogitsProcessor
by tests/test_whisper_timestamps_ref.py).  Every case prints its distances before it asserts.

Bars.  u = 2^-24.
* ssak_dec_timestamp_step.  Tokens, finished flags, n_unfinished, ts_last, h_next: exact.  Log-probabilities: TWICE the bar of
  tests/test_gpu_whisper_generate.py::test_greedy_step_planted_rows over the columns of the final processed row -- rel = (4 D + K
  + 6) u with D = max_c |x_c - max x|, K = ceil(n / 256) + 10, bar = rel + 2 u (|log s| + |m| + |lse|) + 2 u (|x_t| + |logprob|) --
  the same two-pass sum with one more logarithm (the mass decision's) and a maximum M that may lie above the final row's.
  The planted rows keep the decision margin |log S_ts - (m_text - M)| and the final row's top-two gap at 0.5 or more, far beyond
  what fp32 can flip.
* generate / transcribe against the project's own teacher-forced pass: a device token must equal the float64 rule's token on
  the teacher-forced logits unless that rule's own decision margin or top-two gap is below 2 x 7.76e-2 (each path is within
  7.76e-2 of float64: DESIGN.md "Whisper decoder").  no_speech_prob: 7.76e-2 on its logarithm.
"""
import json
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_whisper_dec as G  # noqa: E402
import whisper_decoder_ref as WR  # noqa: E402
import whisper_timestamps_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
LP_BAR = 7.76e-2
V, LDV, EOS, PAD, NOTS, TSB = 127, 128, G.EOT, 3, G.NO_TIMESTAMPS, G.NO_TIMESTAMPS + 1
De, MAXP = 136, 16


@pytest.fixture(scope="module")
def hip():
    import ssak_amd.hip as hip
    return hip


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


@pytest.fixture(scope="module")
def tables():
    g = torch.Generator().manual_seed(31)
    return torch.randn(V, De, generator=g).to(torch.bfloat16), torch.randn(MAXP, De, generator=g).to(torch.bfloat16)


def mask_of(ids, n=V):
    m = np.zeros(n, np.uint8)
    m[list(ids)] = 1
    return torch.from_numpy(m).to(DEV)


def launch(hip, x, hists, was, ts_in, t, tables, sup=(), bsup=(), max_initial=-1, next_pos=5, ldt=8):
    """One launch at step ``t`` on rows whose histories (length t each) sit in the token buffer -> dict of what the kernel wrote."""
    R = x.shape[0]
    E, Pz = tables
    tokens = torch.full((R, ldt), -5, dtype=torch.int32)
    for r, h in enumerate(hists):
        assert len(h) == t
        tokens[r, :t] = torch.tensor(h, dtype=torch.int32)
    before = tokens.clone()
    tokens = tokens.to(DEV)
    lps = torch.full((R, ldt), 9.0, dtype=torch.float32, device=DEV)
    fin = torch.from_numpy(np.asarray(was, dtype=np.uint8)).to(DEV)
    n_unf = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    ts_last = torch.tensor(ts_in, dtype=torch.int32, device=DEV)
    h_next = torch.full((R, De), float("nan"), dtype=torch.bfloat16, device=DEV)
    hip.dec_timestamp_step(x.to(DEV), V, finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, t=t, eos_id=EOS, pad_id=PAD, ts_begin=TSB,
                           no_timestamps_id=NOTS, ts_last=ts_last, max_initial=max_initial, suppress=mask_of(sup) if sup else None,
                           begin_suppress=mask_of(bsup) if bsup else None, first=t == 0, embed_tokens=E.to(DEV), embed_positions=Pz.to(DEV),
                           next_pos=next_pos, h_next=h_next)
    torch.cuda.synchronize()
    tk = tokens.cpu()
    other = [c for c in range(ldt) if c != t]
    assert torch.equal(tk[:, other], before[:, other]) and bool((lps[:, other] == 9.0).all()), "only column t is written"
    return dict(tok=tk[:, t].numpy(), lp=lps[:, t].double().cpu().numpy(), fin=fin.cpu().numpy().astype(bool), n_unf=int(n_unf.item()),
                ts_last=ts_last.cpu().numpy(), h_next=h_next.cpu())


def lp_bar(x64, row):
    """Twice the greedy step's bar on the final processed row ``row['mask']`` of logits x64 [V]."""
    xs = x64[row["mask"]]
    m = xs.max()
    Dm = np.abs(xs - m).max()
    s = np.exp(xs - m).sum()
    rel = (4 * Dm + math.ceil(V / 256) + 10 + 6) * U
    x_t = x64[row["token"]]
    return 2 * (rel + 2 * U * (abs(np.log(s)) + abs(m) + abs(m + np.log(s))) + 2 * U * (abs(x_t) + abs(row["logprob"])))


def check_launch(got, x, hists, was, ts_in, tables, name, sup=(), bsup=(), max_initial=None, next_pos=5, planted=True):
    E, Pz = tables
    x64 = x[:, :V].double().numpy()
    want_tok, want_lp, want_fin, rows = TR.timestamp_step(x64, hists, was, EOS, PAD, TSB, NOTS, max_initial, list(sup), list(bsup))
    worst = 0.0
    for r, row in enumerate(rows):
        if row is None:
            assert got["tok"][r] == PAD and got["lp"][r] == 0.0 and got["ts_last"][r] == ts_in[r], "a finished row: pad, 0, ts_last untouched"
            continue
        if planted:
            assert row["margin"] >= 0.5 and (row["gap"] >= 0.5 or row["gap"] == 0.0), (name, r, row["margin"], row["gap"])
        assert got["ts_last"][r] == row["ts_last"], (name, r, got["ts_last"][r], row["ts_last"])
        err, bar = abs(got["lp"][r] - row["logprob"]), lp_bar(x64[r], row)
        worst = max(worst, err / bar)
        assert err <= bar, (name, r, err, bar)
    print(f"timestamp step {name}: tokens {got['tok'].tolist()}, ts_last {got['ts_last'].tolist()}, worst log-prob err / bar {worst:.3f} "
          f"(max err {np.abs(got['lp'] - want_lp).max():.3e})")
    assert np.array_equal(got["tok"], want_tok), (name, got["tok"], want_tok)
    assert np.array_equal(got["fin"], want_fin) and got["n_unf"] == int((~want_fin).sum())
    want_h = (E[torch.from_numpy(want_tok)].float() + Pz[next_pos].float()[None]).to(torch.bfloat16)
    assert torch.equal(got["h_next"].view(torch.int16), want_h.view(torch.int16)), "h_next is defined bit for bit"
    return want_tok, rows


def base_rows(R, seed):
    x = torch.randn(R, LDV, generator=torch.Generator().manual_seed(seed))
    x[:, V:] = 1e30
    return x


# ------------------------------------------------------------------------------------------------------------ 1. planted rows
def test_timestamp_step_planted_rows(hip, tables):
    """One row per rule state, V = 127 in 128 columns with +1e30 in the pad column; rows grouped by step t (one launch each).

    t = 0 (first, both suppress masks, max_initial 5, ts_last pre-filled with junk that must not be read): the row maximum on a
    text column; on a timestamp beyond max_initial; on a suppressed and on a begin-suppressed timestamp inside the range; on
    <|notimestamps|>; a finished row.
    t = 1 after [ts]: timestamps masked although they dominate; an eos row.
    t = 2 after [ts, text]: timestamp mass dominant while the single best column is text (token >= ts_last + 1, log-prob over
    the timestamps only); text dominant; the row maximum on <|notimestamps|>; an exact tie between two timestamps.
    t = 3 after [ts, text, ts]: text below eos masked although it dominates and the timestamp equal to ts_last chosen; eos chosen.
    t = 4 after [ts, text, ts, ts]: timestamps masked, text chosen."""
    # ---- t = 0
    x = base_rows(6, 41)
    x[0, 17] = 12.0
    x[0, TSB + 2] = 6.0
    x[1, TSB + 9] = 12.0
    x[1, TSB + 5] = 6.0
    x[2, TSB + 1] = 12.0  # suppressed
    x[2, TSB + 3] = 9.0   # begin-suppressed
    x[2, TSB + 0] = 6.0
    x[3, NOTS] = 12.0
    x[3, TSB + 4] = 6.0
    x[4, TSB + 1] = 12.0  # (finished)
    x[5, TSB + 4] = 6.0
    x[5, EOS] = 12.0      # eos is text: not at t = 0
    sup, bsup = [TSB + 1, 50], [TSB + 3, 60]
    was, ts_in = [0, 0, 0, 0, 1, 0], [120, 121, 122, 123, 77, 125]
    got = launch(hip, x, [[]] * 6, was, ts_in, 0, tables, sup, bsup, max_initial=5)
    tok, _ = check_launch(got, x, [[]] * 6, was, ts_in, tables, "t=0", sup, bsup, 5)
    assert tok.tolist() == [TSB + 2, TSB + 5, TSB, TSB + 4, PAD, TSB + 4] and got["ts_last"].tolist() == [TSB + 2, TSB + 5, TSB, TSB + 4, 77, TSB + 4]
    # ---- t = 1, after [ts]
    x = base_rows(2, 42)
    x[0, TSB + 6:V] = 12.0
    x[0, 33] = 6.0
    x[1, EOS] = 9.0
    hists, ts_in = [[TSB + 2], [TSB + 2]], [TSB + 2, TSB + 2]
    got = launch(hip, x, hists, [0, 0], ts_in, 1, tables)
    tok, _ = check_launch(got, x, hists, [0, 0], ts_in, tables, "t=1")
    assert tok.tolist() == [33, EOS] and got["fin"].tolist() == [False, True] and got["ts_last"].tolist() == ts_in
    # ---- t = 2, after [ts, text]
    x = base_rows(4, 43)
    x[0, 40] = 8.0                       # the single best column is text ...
    x[0, TSB:V] = 6.2                    # ... the allowed timestamps (TSB + 5 ..) together outweigh it: 10 e^-1.8 + e^-1 = 2.02
    x[0, TSB + 7] = 7.0
    x[0, TSB + 1] = 30.0                 # below ts_last + 1: masked
    x[1, 40] = 12.0
    x[2, NOTS] = 20.0
    x[2, 41] = 9.0
    x[3, TSB + 8] = x[3, TSB + 12] = 9.0  # an exact tie: the lower id
    hists, ts_in = [[TSB + 4, 7]] * 4, [TSB + 4] * 4
    got = launch(hip, x, hists, [0] * 4, ts_in, 2, tables)
    tok, rows = check_launch(got, x, hists, [0] * 4, ts_in, tables, "t=2")
    assert tok.tolist() == [TSB + 7, 40, 41, TSB + 8] and got["ts_last"].tolist() == [TSB + 7, TSB + 4, TSB + 4, TSB + 8]
    assert not rows[0]["mask"][:TSB].any() and rows[0]["mask"][TSB + 5:].all() and not rows[0]["mask"][TSB:TSB + 5].any()
    # ---- t = 3, after [ts, text, ts]
    x = base_rows(2, 44)
    x[0, 40] = 15.0         # text below eos: masked
    x[0, TSB + 2] = 14.0    # below ts_last: masked
    x[0, TSB + 6] = 9.0     # = ts_last: allowed, chosen
    x[1, EOS] = 12.0
    hists, ts_in = [[TSB + 4, 7, TSB + 6]] * 2, [TSB + 6] * 2
    got = launch(hip, x, hists, [0, 0], ts_in, 3, tables)
    tok, _ = check_launch(got, x, hists, [0, 0], ts_in, tables, "t=3")
    assert tok.tolist() == [TSB + 6, EOS] and got["fin"].tolist() == [False, True]
    # ---- t = 4, after [ts, text, ts, ts]
    x = base_rows(1, 45)
    x[0, TSB + 9] = 12.0
    x[0, 21] = 6.0
    hists, ts_in = [[TSB + 4, 7, TSB + 6, TSB + 6]], [TSB + 6]
    got = launch(hip, x, hists, [0], ts_in, 4, tables)
    tok, _ = check_launch(got, x, hists, [0], ts_in, tables, "t=4")
    assert tok.tolist() == [21] and got["ts_last"].tolist() == [TSB + 6]


# ------------------------------------------------------------------------------------------------------------ 2. six steps
def test_timestamp_step_six_consecutive_steps(hip, tables):
    """Six steps on ONE token buffer: the kernel reads its own tokens at t - 1 and t - 2 and its own ts_last, the restatement is
    fed the growing history.  Per step and row the logits are drawn until the restatement's decision margin and top-two gap are
    at least 0.05 (fp32 moves either by about 1e-6); row 3 is given a dominant eos at step 3 and pads afterwards.  The specials
    between eos and <|notimestamps|> are suppressed, as Whisper's own list does, so that the grammar of the histories holds."""
    R, steps = 4, 6
    sup = list(range(EOS + 1, NOTS))
    E, Pz = tables
    rng = np.random.default_rng(46)
    tokens = torch.full((R, steps), -5, dtype=torch.int32, device=DEV)
    lps = torch.zeros((R, steps), dtype=torch.float32, device=DEV)
    fin = torch.zeros(R, dtype=torch.uint8, device=DEV)
    n_unf = torch.zeros(1, dtype=torch.int32, device=DEV)
    ts_last = torch.full((R,), 99, dtype=torch.int32, device=DEV)
    h_next = torch.empty((R, De), dtype=torch.bfloat16, device=DEV)
    hists, finished, kinds = [[] for _ in range(R)], np.zeros(R, dtype=bool), set()
    for t in range(steps):
        x = np.zeros((R, LDV), dtype=np.float32)
        x[:, V:] = 1e30
        for r in range(R):
            while True:
                x[r, :V] = (2.0 * rng.standard_normal(V)).astype(np.float32)
                x[r, TSB:V] += np.float32(rng.uniform(-1.0, 5.0))
                if r == 3 and t == 3:
                    x[r, EOS] = 30.0
                row = TR.timestamp_step_row(x[r, :V], hists[r], TSB, NOTS, EOS, 5, sup)
                if finished[r] or (row["margin"] >= 0.05 and row["gap"] >= 0.05):
                    break
        want_tok, want_lp, want_fin, rows = TR.timestamp_step(x[:, :V].astype(np.float64), hists, finished, EOS, PAD, TSB, NOTS, 5, sup)
        hip.dec_timestamp_step(torch.from_numpy(x).to(DEV), V, finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, t=t, eos_id=EOS,
                               pad_id=PAD, ts_begin=TSB, no_timestamps_id=NOTS, ts_last=ts_last, max_initial=5, suppress=mask_of(sup), first=t == 0,
                               embed_tokens=E.to(DEV), embed_positions=Pz.to(DEV), next_pos=t + 3, h_next=h_next)
        torch.cuda.synchronize()
        got_tok, got_ts = tokens[:, t].cpu().numpy(), ts_last.cpu().numpy()
        want_ts = [TR.last_timestamp(h + [int(k)], TSB) if not f else TR.last_timestamp(h, TSB) for h, k, f in zip(hists, want_tok, finished)]
        err = np.abs(lps[:, t].double().cpu().numpy() - want_lp).max()
        print(f"step {t}: tokens {got_tok.tolist()} ts_last {got_ts.tolist()} log-prob err {err:.3e}")
        assert np.array_equal(got_tok, want_tok), (t, got_tok, want_tok)
        assert got_ts.tolist() == want_ts and np.array_equal(fin.cpu().numpy().astype(bool), want_fin) and int(n_unf.item()) == int((~want_fin).sum())
        assert err < 1e-5
        for r in range(R):
            if not finished[r]:
                hists[r].append(int(want_tok[r]))
                kinds.add("ts" if want_tok[r] >= TSB else "text")
        finished = want_fin
    assert finished.tolist() == [False, False, False, True] and tokens[3].tolist()[3:] == [EOS, PAD, PAD] and kinds == {"ts", "text"}
    for r in range(3):
        TR.check_grammar(hists[r], TSB, EOS, NOTS, 5)


# ------------------------------------------------------------------------------------------------------------ 3. the vocabulary's width
def test_timestamp_step_vocabulary_width(hip):
    """V = 51 865 in a 51 872-column buffer, ts_begin 50 364: after [ts, text] row 1's maximum sits in the LAST timestamp column, the
    one-column tail behind the vector loop; row 0's on a text column that outweighs the 1501 timestamps."""
    Vw, ldv, tsb, nots, eos = 51865, 51872, 50364, 50363, 50257
    x = 3 * torch.randn(2, ldv, generator=torch.Generator().manual_seed(47))
    x[:, Vw:] = 1e30
    x[0, 1000] = 40.0
    x[1, Vw - 1] = 40.0
    tokens = torch.full((2, 3), -5, dtype=torch.int32)
    tokens[:, 0], tokens[:, 1] = tsb + 10, 500
    tokens = tokens.to(DEV)
    lps = torch.zeros((2, 3), dtype=torch.float32, device=DEV)
    fin, n_unf = torch.zeros(2, dtype=torch.uint8, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ts_last = torch.full((2,), tsb + 10, dtype=torch.int32, device=DEV)
    hip.dec_timestamp_step(x.to(DEV), Vw, finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, t=2, eos_id=eos, pad_id=eos, ts_begin=tsb,
                           no_timestamps_id=nots, ts_last=ts_last, max_initial=50)
    torch.cuda.synchronize()
    want_tok, want_lp, _, rows = TR.timestamp_step(x[:, :Vw].double().numpy(), [[tsb + 10, 500]] * 2, [False, False], eos, eos, tsb, nots, 50)
    err = np.abs(lps[:, 2].double().cpu().numpy() - want_lp)
    print(f"timestamp step V={Vw}: tokens {tokens[:, 2].tolist()}, margins {[r['margin'] for r in rows]}, log-prob err {err.max():.3e}")
    assert tokens[:, 2].tolist() == want_tok.tolist() == [1000, Vw - 1] and err.max() < 1e-4
    assert ts_last.tolist() == [tsb + 10, Vw - 1] and int(n_unf.item()) == 2


# ------------------------------------------------------------------------------------------------------------ 4. refusals
def test_timestamp_step_refusals(hip, tables):
    E, Pz = tables
    R = 3
    x = base_rows(R, 48).to(DEV)
    tokens = torch.full((R, 3), -5, dtype=torch.int32, device=DEV)
    lps = torch.zeros((R, 3), dtype=torch.float32, device=DEV)
    fin = torch.zeros(R, dtype=torch.uint8, device=DEV)
    n_unf = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    ts_last = torch.full((R,), 55, dtype=torch.int32, device=DEV)
    h_next = torch.full((R, De), 7.0, dtype=torch.bfloat16, device=DEV)
    kw = dict(finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, embed_tokens=E.to(DEV), embed_positions=Pz.to(DEV), h_next=h_next)
    ok = dict(t=0, eos_id=EOS, pad_id=PAD, ts_begin=TSB, no_timestamps_id=NOTS, ts_last=ts_last, next_pos=0)
    for change, match in ((dict(ts_begin=EOS), "ts_begin"), (dict(ts_begin=V), "ts_begin"), (dict(no_timestamps_id=V), "no_timestamps_id"),
                          (dict(no_timestamps_id=-1), "no_timestamps_id"), (dict(ts_last=None), "ts_last"), (dict(next_pos=MAXP), "overruns"),
                          (dict(eos_id=V), "eos_id"), (dict(pad_id=-1), "pad_id"), (dict(t=3), "step t")):
        with pytest.raises(ValueError, match=match):
            hip.dec_timestamp_step(x, V, **dict(ok, **change), **kw)
    torch.cuda.synchronize()
    assert bool((tokens == -5).all()) and int(n_unf.item()) == 77 and bool((h_next == 7.0).all()) and bool((ts_last == 55).all()) \
        and bool((fin == 0).all()), "a refused call launched"


# ------------------------------------------------------------------------------------------------------------ 5. generate
B = 3
MAX_INITIAL = 5
KEEP = sorted(np.random.default_rng(7).choice(100, size=10, replace=False).tolist())  # the text ids left open (seed 7: see the test below)
SUPPRESS = list(range(G.SOT, NOTS + 1)) + [t for t in range(EOS) if t not in KEEP]     # every special but eos, 90 of the 100 text ids


@pytest.fixture(scope="module")
def model(golden):
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq, WhisperSeq2SeqConfig
    gen = json.loads(str(golden["generation_config_json"]))
    cfg = WhisperSeq2SeqConfig.from_hf_dict(json.loads(str(golden["config_json"])),
                                            lang_to_id={str(c): int(i) for c, i in zip(golden["lang_codes"], golden["lang_ids"])},
                                            task_to_id=gen["task_to_id"], no_timestamps_token_id=gen["no_timestamps_token_id"],
                                            max_initial_timestamp_index=MAX_INITIAL)
    m = WhisperSeq2Seq(cfg)
    m.load_decoder_state_dict({k[2:]: torch.from_numpy(WR.bf16_from_bits(golden[k]).astype(np.float32)) for k in golden.files if k.startswith("w/")})
    return m


@pytest.fixture(scope="module")
def enc(golden):
    return torch.from_numpy(WR.bf16_from_bits(golden["enc"]).astype(np.float32)).to(torch.bfloat16)


def near_tie_share(model, enc_out, prompt, token_rows, enc_lens, suppress, max_initial, ts_begin, nots, eos):
    """Teacher-forced check of free-run tokens: ``token_rows[b]`` = utterance b's tokens (through its eos).  -> (steps, exempt
    steps); asserts that every other step's token is the float64 rule's on the teacher-forced logits."""
    n = max(len(r) for r in token_rows)
    full = np.full((len(token_rows), prompt.shape[1] + n), eos, dtype=np.int64)
    full[:, :prompt.shape[1]] = prompt
    for b, r in enumerate(token_rows):
        full[b, prompt.shape[1]:prompt.shape[1] + len(r)] = r
    logits = model.decode_logits(enc_out, full, enc_lens).double().cpu().numpy()
    P = prompt.shape[1]
    steps = exempt = 0
    for b, r in enumerate(token_rows):
        for i, tok in enumerate(r):
            row = TR.timestamp_step_row(logits[b, P - 1 + i], list(r[:i]), ts_begin, nots, eos, max_initial, suppress)
            steps += 1
            if row["margin"] < 2 * LP_BAR or row["gap"] < 2 * LP_BAR:
                exempt += 1
                continue
            assert tok == row["token"], (b, i, tok, row["token"], row["margin"], row["gap"])
    return steps, exempt


def test_generate_with_timestamps(model, enc, golden):
    """``generate(timestamps=True)`` on the tiny fixture (16 timestamp tokens, max_initial 5): default prompt [sot, language,
    task], 16 = 32 // 2 tokens at most.  Grammar outright; teacher-forced consistency with the float64 rule.

    The suppress list leaves eos and 10 of the 100 text ids open (the draw of seed 7).  On the CPU the float64 restatement alone
    (whisper_timestamps_ref.generate on whisper_decoder_ref) gives lens (2, 16, 16) and 2 of its 34 steps (5.9 %) below the
    2 x 7.76e-2 bar, the smallest of them at 0.140; with the specials alone suppressed the share is 14 of 48 (29 %), which is why
    the list is what it is.  At most 10 % of the device's steps may be exempt."""
    enc_lens = golden["enc_lens"]
    r = model.generate(enc, enc_lens=enc_lens, suppress_tokens=SUPPRESS, timestamps=True)
    print(f"generate(timestamps=True): tokens {r.tokens}, no_speech_prob {r.no_speech_prob}")
    assert r.token_array.shape[1] <= 16 and r.no_speech_prob is not None and r.no_speech_prob.shape == (B,)
    for toks in r.tokens:
        TR.check_grammar(toks, TSB, EOS, NOTS, MAX_INITIAL)
        assert not np.isin(toks, SUPPRESS).any()
    codes, _ = model.detect_language(enc, enc_lens)
    prompt = model.default_prompt(B, codes, timestamps=True)
    assert prompt.shape == (B, 3) and prompt[0].tolist() == [G.SOT, G.LANG0 + G.LANGS.index(codes[0]), G.TRANSCRIBE]
    steps, exempt = near_tie_share(model, enc, prompt, r.tokens, enc_lens, SUPPRESS, MAX_INITIAL, TSB, NOTS, EOS)
    print(f"teacher-forced: {exempt} of {steps} steps below the 2 x {LP_BAR} bar (exempt)")
    assert exempt <= 0.10 * steps
    for poll_every in (0, 1, 8):
        rp = model.generate(enc, enc_lens=enc_lens, suppress_tokens=SUPPRESS, timestamps=True, poll_every=poll_every)
        assert rp.tokens == r.tokens and np.array_equal(rp.logprobs[:, :r.logprobs.shape[1]], r.logprobs), poll_every
    # no_speech_prob: the softmax of the <|startoftranscript|> row, against float64 on the fixture's weights
    w = {k[2:]: WR.bf16_from_bits(golden[k]) for k in golden.files if k.startswith("w/")}
    enc64 = WR.bf16_from_bits(golden["enc"])
    d = 0.0
    for b in range(B):
        lg = WR.decoder_logits(w, G.NH, G.LAYERS, enc64[b:b + 1, :int(enc_lens[b])], np.array([[G.SOT]]))[0, 0]
        want = (lg[NOTS - 1] - lg.max()) - np.log(np.exp(lg - lg.max()).sum())
        d = max(d, abs(np.log(r.no_speech_prob[b]) - want))
    print(f"no_speech_prob: max |log difference| to float64 {d:.3e} (bar {LP_BAR})")
    assert d <= LP_BAR


def test_generate_default_is_unchanged(model, enc, golden, hip):
    """Without ``timestamps=`` the call is the greedy one bit for bit: the same tokens and log-probabilities as the loop written
    out with ``ssak_dec_greedy_step`` on the stepping primitives, and no no_speech_prob."""
    sup = list(range(EOS, NOTS + 1))
    enc_lens = golden["enc_lens"]
    a = model.generate(enc, max_new_tokens=6, enc_lens=enc_lens, suppress_tokens=sup)
    b = model.generate(enc, max_new_tokens=6, enc_lens=enc_lens, suppress_tokens=sup, timestamps=False)
    assert a.no_speech_prob is None and a.tokens == b.tokens and np.array_equal(a.logprobs, b.logprobs)
    codes, _ = model.detect_language(enc, enc_lens)
    prompt = model.default_prompt(B, codes)
    assert prompt.shape == (B, 4) and (prompt[:, 3] == NOTS).all()
    st = model._gen_begin(enc.to(DEV), enc_lens, cap=4 + 6)
    logits = model._gen_prefill(st, prompt)
    E, Pz = model._w("embed_tokens.weight"), model._w("embed_positions.weight")
    tokens = torch.zeros((B, 6), dtype=torch.int32, device=DEV)
    lps = torch.zeros((B, 6), dtype=torch.float32, device=DEV)
    fin, n_unf = torch.zeros(B, dtype=torch.uint8, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    h_next = torch.empty((B, st.D), dtype=torch.bfloat16, device=DEV)
    for i in range(6):
        hip.dec_greedy_step(logits, G.V, finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, t=i, eos_id=EOS, pad_id=EOS,
                            suppress=model._token_mask(sup, "s"), first=i == 0, embed_tokens=E, embed_positions=Pz, next_pos=4 + i,
                            h_next=None if i == 5 else h_next)
        if i < 5:
            logits = model._gen_step(st, h_next)
    assert np.array_equal(tokens.cpu().numpy(), a.token_array) and np.array_equal(lps.double().cpu().numpy(), a.logprobs)


# ------------------------------------------------------------------------------------------------------------ 6. transcribe
VT = 111 + 1501  # the fixture's id layout with Whisper's 1501 timestamps (0.00 .. 30.00 s)
SUPPRESS_T = list(range(G.SOT, NOTS + 1))
SECONDS = (5, 31, 47)


@pytest.fixture(scope="module")
def long_weights():
    """A seeded model of the test's own, drawn as gen_golden_whisper_dec.draw does: d_model 128, 2 heads, 1 encoder layer, 2 decoder
    layers, ffn 256, 1500 source positions, 32 target positions, V = 111 + 1501."""
    rng = np.random.default_rng(62)
    shapes = G.decoder_param_shapes()
    shapes["model.decoder.embed_tokens.weight"] = (VT, G.D)
    w = G.draw(shapes, rng)
    w.update(G.draw(G.encoder_param_shapes(1500, 1), rng))
    return w


def long_generation_config():
    return dict(G.generation_config_dict(), suppress_tokens=SUPPRESS_T, begin_suppress_tokens=[EOS], max_initial_timestamp_index=50)


@pytest.fixture(scope="module")
def long_model(long_weights):
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq, WhisperSeq2SeqConfig
    gen = long_generation_config()
    cfg = WhisperSeq2SeqConfig.from_hf_dict(dict(G.config_dict(1500, 1), vocab_size=VT),
                                            lang_to_id={c: G.LANG0 + i for i, c in enumerate(G.LANGS)},
                                            **{k: gen[k] for k in ("task_to_id", "no_timestamps_token_id", "suppress_tokens", "begin_suppress_tokens",
                                                                   "max_initial_timestamp_index")})
    m = WhisperSeq2Seq(cfg)
    t = {k: torch.from_numpy(v.astype(np.float32)) for k, v in long_weights.items()}
    m.encoder.load_state_dict({k[len("model."):]: v for k, v in t.items() if k.startswith("model.encoder.")}, strict=False)
    m.load_decoder_state_dict(t)
    return m


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(63)
    return [torch.from_numpy((0.1 * rng.standard_normal(16000 * s)).astype(np.float32)) for s in SECONDS]


def window_audio(wave_, seek):
    w = torch.zeros(480000)
    part = wave_[seek * 160:seek * 160 + 480000]
    w[:part.numel()] = part
    return w[None]


def test_transcribe_long_form(long_model, noise):
    from ssak_amd.whisper_transcribe import segments_from_window
    m = long_model
    rounds = []
    gen = m.generate

    def counting(enc_out, **kw):
        rounds.append(enc_out.shape[0])
        return gen(enc_out, **kw)

    m.generate = counting
    try:
        res = m.transcribe(noise, _max_rounds=64)
    finally:
        del m.generate
    print(f"transcribe: batch per round {rounds}; seeks {[r.seeks for r in res]}; segments {[len(r.segments) for r in res]}; "
          f"languages {[r.language for r in res]}")
    assert rounds[0] == 3 and rounds[1] == 2 and all(a >= b for a, b in zip(rounds, rounds[1:])), "the 5 s file leaves after round one"
    ts_begin = NOTS + 1
    for r, s in zip(res, SECONDS):
        assert r.content_frames == s * 100 and r.seeks[0] == 0 and r.seeks[-1] == r.content_frames
        assert all(a < b for a, b in zip(r.seeks, r.seeks[1:])) and len(r.windows) == len(r.seeks) - 1 and r.language in G.LANGS
        segs = []
        for w, nxt in zip(r.windows, r.seeks[1:]):
            assert w.segment_frames == min(3000, r.content_frames - w.seek) and 0.0 <= w.no_speech_prob <= 1.0
            TR.check_grammar(w.tokens, ts_begin, EOS, NOTS, 50)
            assert not np.isin(w.tokens, SUPPRESS_T).any() and len(w.tokens) <= 16
            sg, new_seek = segments_from_window(w.tokens, w.seek, w.segment_frames, ts_begin, EOS, 2, w.avg_logprob, w.no_speech_prob, 0.6, -1.0)
            assert min(new_seek, r.content_frames) == nxt
            segs += sg
        assert segs == r.segments
        for sg in r.segments:
            assert 0.0 <= sg.start < sg.end and any(t < EOS for t in sg.tokens)
    assert len(res[0].windows) == 1 and sum(len(r.segments) for r in res) >= 1
    # the order of the files changes nothing
    perm = m.transcribe([noise[2], noise[0], noise[1]], _max_rounds=64)
    for a, b in zip(res, (perm[1], perm[2], perm[0])):
        assert a.seeks == b.seeks and [w.tokens for w in a.windows] == [w.tokens for w in b.windows] and a.language == b.language
    # each file alone against the batch: identical, or the first difference is a near-tie on teacher-forced logits
    for f, (r, wv) in enumerate(zip(res, noise)):
        alone = m.transcribe([wv], language=r.language, _max_rounds=64)[0]
        for wa, wb in zip(alone.windows, r.windows):
            assert wa.seek == wb.seek
            if wa.tokens == wb.tokens:
                continue
            i = next(k for k, (x, y) in enumerate(zip(wa.tokens + [EOS], wb.tokens + [EOS])) if x != y)
            enc_out = m.encode(m.features(window_audio(wv, wa.seek)))
            prompt = m.default_prompt(1, r.language, timestamps=True)
            full = np.concatenate([prompt, np.array([wb.tokens[:i] + [EOS]])], 1)
            lg = m.decode_logits(enc_out, full).double().cpu().numpy()[0, prompt.shape[1] - 1 + i]
            row = TR.timestamp_step_row(lg, wb.tokens[:i], ts_begin, NOTS, EOS, 50, SUPPRESS_T, [EOS])
            print(f"file {f} window at {wa.seek}: alone and in the batch differ at step {i}; margin {row['margin']:.3e}, gap {row['gap']:.3e}")
            assert row["margin"] < 2 * LP_BAR or row["gap"] < 2 * LP_BAR
            break
        else:
            assert alone.seeks == r.seeks
    with pytest.raises(RuntimeError, match="rounds"):
        m.transcribe([noise[1]], language="en", _max_rounds=1)


# ------------------------------------------------------------------------------------------------------------ 7. the command line
class _Stored:
    """What gen_golden_whisper_dec.write_folder reads of an npz: ``files``, ``w/<name>`` bf16 bit patterns, the generation config."""

    def __init__(self, weights, generation_config):
        self.d = {"w/" + k: WR.bf16_bits(v) for k, v in weights.items() if k.startswith("model.decoder.")}
        self.d["generation_config_json"] = json.dumps(generation_config)
        self.files = list(self.d)

    def __getitem__(self, k):
        return self.d[k]


def test_command_line_timestamps(long_weights, noise, tmp_path, capsys):
    from ssak_amd import whisper_infer
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq
    folder = G.write_folder(_Stored(long_weights, long_generation_config()), str(tmp_path / "model"), max_source_positions=1500, encoder_layers=1,
                            config_overrides={"vocab_size": VT})
    path = str(tmp_path / "noise31.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1), f.setsampwidth(2), f.setframerate(16000)
        f.writeframes((noise[1].numpy() * 32767).astype("<i2").tobytes())
    whisper_infer.main([path, "--model", folder, "--language", "en", "--timestamps"])
    lines = capsys.readouterr().out.strip().splitlines()
    from ssak_amd.data import load_audio
    want = WhisperSeq2Seq.from_pretrained(folder).transcribe([torch.from_numpy(load_audio(path))], language="en")[0].segments
    print(f"--timestamps: {len(lines)} lines, first {lines[:1]}")
    assert len(lines) == len(want) >= 1
    for line, sg in zip(lines, want):
        p, a, b, ids = line.split("\t")[:4]
        assert p == path and float(a) == round(sg.start, 2) and float(b) == round(sg.end, 2) and 0.0 <= float(a) < float(b) <= 31.0 + 30.0
        assert [int(t) for t in ids.split()] == [t for t in sg.tokens if t < NOTS + 1]
    with pytest.raises(SystemExit, match="30 s"):
        whisper_infer.main([path, "--model", folder, "--language", "en"])
