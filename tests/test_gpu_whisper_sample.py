"""GPU: Whisper sampling and temperature fallback -- ssak_dec_sample_step (ssak_amd/csrc/whisper_generate.hip),
``WhisperSeq2Seq.generate(temperature=..., best_of=..., seed=...)`` (ssak_amd/whisper_seq2seq.py), the fallback of
``WhisperSeq2Seq.transcribe`` (ssak_amd/whisper_transcribe.py) and ``python -m ssak_amd.whisper_infer --accurate`` -- against the
float64 restatement tests/whisper_sample_ref.py (held to softmax(x / T) by tests/test_whisper_sample_ref.py).  The layout and the
fixtures are those of tests/test_gpu_whisper_timestamps.py.  Every case prints its distances before it asserts.

Bars.  u = 2^-24.
* ssak_dec_sample_step, tokens.  The draw is the arg-max of x / T + g with the restatement's own noise; the device token must lie
  in the restatement's accept set (the columns within delta_c + delta_argmax of the float64 maximum, delta_c = u (4 |x_c / T| +
  7 |g_c| + 6): whisper_sample_ref's docstring).  The planted rows keep the top-two score gap at 1e-3 or more, asserted, so their
  accept set is one column and the token is compared exactly; with the rules they keep the mass decision's margin at 0.5 or more.
* log-probabilities: the bar of test_gpu_whisper_timestamps.py::test_timestamp_step_planted_rows over the candidate set, evaluated
  at the drawn token -- 2 (rel + 2 u (|log s| + |m| + |lse|) + 2 u (|x_t| + |logprob|)), rel = (4 D + ceil(n / 256) + 16) u, D =
  max_c |x_c - max x| over the finite candidates.  finished, n_unfinished, ts_last, h_next: exact; only column t is written.
* generate: a device token must equal the float64 rule's token (same noise) on the project's teacher-forced logits of the
  device's own history unless that rule's top-two score gap is below 2 x 7.76e-2 / T (each path's logits are within 7.76e-2 of
  float64, DESIGN.md "Whisper decoder"; the division by T carries it into the scores); at most a quarter of the steps may be
  excused (the float64 decoder alone excuses at most an eighth at this seed: tests/test_whisper_sample_ref.py).
"""
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
import test_gpu_whisper_timestamps as T  # noqa: E402
import whisper_generate_ref as GR  # noqa: E402
import whisper_sample_ref as SR  # noqa: E402
import whisper_timestamps_ref as TR  # noqa: E402
from test_gpu_whisper_timestamps import enc, golden, hip, long_model, long_weights, model, noise, tables  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV, U = T.DEV, T.U
V, LDV, EOS, PAD, NOTS, TSB, De, MAXP = T.V, T.LDV, T.EOS, T.PAD, T.NOTS, T.TSB, T.De, T.MAXP
SEED = 0x5EED5A3D1E5
ALL = list(range(V))


def launch(hip, x, t, temperature, seed, tables=None, hists=None, was=None, ts_in=None, sup=(), bsup=(), max_initial=-1, next_pos=5, ldt=4, Vn=V,
           eos=EOS, pad=PAD, tsb=TSB, nots=NOTS):
    """One ssak_dec_sample_step at step ``t`` on x [R, ldv] (a device or host tensor) -> dict of what the kernel wrote.  ``hists`` (one
    history of length t per row): with the timestamp rules, ``ts_in`` in ts_last; None: no rules (ts_last NULL)."""
    R = x.shape[0]
    tokens = torch.full((R, ldt), -5, dtype=torch.int32)
    if hists is not None:
        for r, h in enumerate(hists):
            assert len(h) == t
            tokens[r, :t] = torch.tensor(h, dtype=torch.int32)
    before = tokens.clone()
    tokens = tokens.to(DEV)
    lps = torch.full((R, ldt), 9.0, dtype=torch.float32, device=DEV)
    fin = torch.from_numpy(np.asarray([0] * R if was is None else was, dtype=np.uint8)).to(DEV)
    n_unf = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    rules = {}
    if hists is not None:
        rules = dict(ts_begin=tsb, no_timestamps_id=nots, max_initial=max_initial, ts_last=torch.tensor(ts_in, dtype=torch.int32, device=DEV))
    emb = {}
    h_next = None
    if tables is not None:
        h_next = torch.full((R, De), float("nan"), dtype=torch.bfloat16, device=DEV)
        emb = dict(embed_tokens=tables[0].to(DEV), embed_positions=tables[1].to(DEV), next_pos=next_pos, h_next=h_next)
    mk = lambda ids: T.mask_of(ids, Vn) if len(ids) else None
    hip.dec_sample_step(x.to(DEV), Vn, finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, t=t, eos_id=eos, pad_id=pad,
                        temperature=temperature, seed=seed, suppress=mk(sup), begin_suppress=mk(bsup), first=t == 0, **rules, **emb)
    torch.cuda.synchronize()
    tk = tokens.cpu()
    other = [c for c in range(ldt) if c != t]
    assert torch.equal(tk[:, other], before[:, other]) and bool((lps[:, other] == 9.0).all()), "only column t is written"
    return dict(tok=tk[:, t].numpy(), lp=lps[:, t].double().cpu().numpy(), lp_bits=lps[:, t].cpu().view(torch.int32).numpy(),
                fin=fin.cpu().numpy().astype(bool), n_unf=int(n_unf.item()), ts_last=rules["ts_last"].cpu().numpy() if rules else None,
                h_next=None if h_next is None else h_next.cpu())


def lp_bar(x64, d, n):
    """The timestamp step's log-prob bar over the finite candidates ``d['mask']`` of logits x64 [n], at the drawn token."""
    xs = x64[d["mask"] & np.isfinite(x64)]
    m = xs.max()
    s = np.exp(xs - m).sum()
    rel = (4 * np.abs(xs - m).max() + math.ceil(n / 256) + 10 + 6) * U
    return 2 * (rel + 2 * U * (abs(np.log(s)) + abs(m) + abs(m + np.log(s))) + 2 * U * (abs(x64[d["token"]]) + abs(d["logprob"])))


def check(got, x, t, temperature, seed, name, tables=None, hists=None, was=None, ts_in=None, sup=(), bsup=(), max_initial=None, next_pos=5,
          planted=True, Vn=V, eos=EOS, pad=PAD, tsb=TSB, nots=NOTS):
    """``got`` of :func:`launch` against the restatement -> (the restatement's tokens, its per-row dicts)."""
    R = x.shape[0]
    x64 = x[:, :Vn].double().cpu().numpy()
    was = [0] * R if was is None else was
    want_tok, want_lp, want_fin, rows = SR.sample_step(x64, was, eos, pad, temperature, seed, t, hists, ts_begin=tsb, no_timestamps=nots,
                                                       max_initial=max_initial, suppress=list(sup), begin_suppress=list(bsup))
    worst, exact = 0.0, True
    for r, d in enumerate(rows):
        if d is None:
            assert got["tok"][r] == pad and got["lp"][r] == 0.0, "a finished row: pad, 0"
            assert hists is None or got["ts_last"][r] == ts_in[r], "a finished row's ts_last is left alone"
            continue
        if d["token"] is None:
            assert got["tok"][r] == pad and got["lp"][r] == 0.0, "a row without a candidate: pad, 0"
            continue
        if planted:
            assert d["gap"] >= 1e-3 and len(d["accept"]) == 1, (name, r, d["gap"])
            if hists is not None:
                margin = TR.timestamp_step_row(x64[r], list(hists[r]), tsb, nots, eos, max_initial, list(sup), list(bsup))["margin"]
                assert margin >= 0.5, (name, r, margin)
        assert got["tok"][r] in d["accept"], (name, r, got["tok"][r], d["accept"], d["gap"])
        if got["tok"][r] != d["token"]:  # (a near-tie inside the accept set: the log-prob is the device token's)
            exact = False
            d = dict(d, token=int(got["tok"][r]), logprob=float(GR.log_softmax(np.where(d["mask"], x64[r], -np.inf)[None])[0, got["tok"][r]]))
            rows[r] = d
        err, bar = abs(got["lp"][r] - d["logprob"]), lp_bar(x64[r], d, Vn)
        worst = max(worst, err / bar)
        assert err <= bar, (name, r, err, bar)
    print(f"sample step {name}: tokens {got['tok'].tolist()[:12]}, gaps {[round(d['gap'], 3) for d in rows if d is not None][:12]}, worst "
          f"log-prob err / bar {worst:.3f}")
    dev_tok = got["tok"]
    if planted:
        assert exact and np.array_equal(dev_tok, want_tok), (name, dev_tok, want_tok)
    fin = np.asarray(was, dtype=bool) | (dev_tok == eos)
    assert np.array_equal(got["fin"], fin) and got["n_unf"] == int((~fin).sum())
    if hists is not None:
        for r, d in enumerate(rows):
            if d is not None:
                prev = -1 if t == 0 else TR.last_timestamp(hists[r], tsb)
                assert got["ts_last"][r] == (dev_tok[r] if d["token"] is not None and dev_tok[r] >= tsb else prev), (name, r)
    if tables is not None:
        E, Pz = tables
        want_h = (E[torch.from_numpy(dev_tok.astype(np.int64))].float() + Pz[next_pos].float()[None]).to(torch.bfloat16)
        assert torch.equal(got["h_next"].view(torch.int16), want_h.view(torch.int16)), "h_next is defined bit for bit"
    return dev_tok, rows


def run(hip, x, t, temperature, name, tables=None, seed=SEED, **kw):
    launch_kw = dict({k: v for k, v in kw.items() if k != "planted"}, max_initial=-1 if kw.get("max_initial") is None else kw["max_initial"])
    got = launch(hip, x, t, temperature, seed, tables, **launch_kw)
    return check(got, x, t, temperature, seed, name, tables, **kw), got


# ------------------------------------------------------------------------------------------------------------ 1. planted rows
@pytest.mark.parametrize("rules", [True, False])
def test_sample_step_planted_rows(hip, tables, rules):
    """One launch per step t = 0, 1, 2 and per special case, with the timestamp rules and without (``ts_last`` NULL: the columns from
    TSB on are text like any other).
    t = 0 (first, both masks, max_initial 5, ts_last pre-filled with junk): a random row, a finished row, a row holding -inf in allowed
    columns.  t = 1 after [ts]: random rows and a dominant eos.  t = 2 after [ts, text], T = 1: the timestamps' mass wins over the
    best single text column (the token is a timestamp, the log-prob over the timestamps alone), loses, a finished row, -inf columns.
    T = 0.01 on rows with a top-two logit gap of 1: the greedy token.  One allowed column: that column, log-prob 0.  No allowed
    column: pad, 0."""
    H = (lambda *h: [list(hh) for hh in h]) if rules else (lambda *h: None)
    ts = lambda *v: list(v) if rules else None
    # ---- t = 0
    x = T.base_rows(3, 141)
    x[2, [TSB, TSB + 2, 5, 6]] = float("-inf")
    sup, bsup = [TSB + 1, 50], [TSB + 3, 60]
    (tok, rows), got = run(hip, x, 0, 1.0, "t=0", tables, hists=H([], [], []), was=[0, 1, 0], ts_in=ts(120, 77, 122), sup=sup, bsup=bsup,
                           max_initial=5 if rules else None)
    assert not np.isin(tok[[0, 2]], sup + bsup).any() and tok[2] not in (TSB, TSB + 2, 5, 6) and tok[1] == PAD
    if rules:
        assert all(TSB <= k <= TSB + 5 for k in tok[[0, 2]]) and got["ts_last"].tolist() == [tok[0], 77, tok[2]]
    # ---- t = 1, after [ts]
    x = T.base_rows(3, 142)
    x[2, EOS] = 12.0
    (tok, rows), got = run(hip, x, 1, 1.0, "t=1", tables, hists=H([TSB + 2], [TSB + 2], [TSB + 2]), ts_in=ts(TSB + 2, TSB + 2, TSB + 2))
    assert tok[2] == EOS and got["fin"].tolist() == [False, False, True]
    if rules:
        assert (tok < TSB).all() and got["ts_last"].tolist() == [TSB + 2] * 3
    # ---- t = 2, after [ts, text]
    x = T.base_rows(4, 143)
    x[0, 40] = 8.0
    x[0, TSB:V] = 6.2
    x[0, TSB + 7] = 7.0
    x[0, TSB + 1] = 30.0  # below ts_last + 1 with the rules (without them it dominates the row)
    x[1, 40] = 12.0
    x[3, 30] = 6.0
    x[3, [41, 42, TSB + 9]] = float("-inf")
    hist = [TSB + 4, 7]
    (tok, rows), got = run(hip, x, 2, 1.0, "t=2", tables, hists=H(hist, hist, hist, hist), was=[0, 0, 1, 0], ts_in=ts(*[TSB + 4] * 4))
    if rules:
        assert tok[0] >= TSB + 5 and not rows[0]["mask"][:TSB].any() and rows[0]["mask"][TSB + 5:].all(), "the mass wins: timestamps alone"
        assert rows[1]["mask"][:EOS].any() and got["ts_last"][0] == tok[0], "the mass loses: every allowed column"
    assert tok[2] == PAD and tok[3] not in (41, 42, TSB + 9)
    # ---- T = 0.01 on a top-two logit gap of 1: the greedy token (the noise spans 19.5, the scores' gap is 100)
    x = T.base_rows(4, 144)
    x[:, TSB:V] -= 3.0  # (the timestamps' mass far below the best text column: the decision is not what this case is about)
    for r in range(4):
        top = int(x[r, :EOS].argmax())
        x[r, top] = x[r, :V].max() + 1.0
    hist4 = H(*[hist] * 4)
    (tok, rows), _ = run(hip, x, 2, 0.01, "T=0.01", tables, hists=hist4, ts_in=ts(*[TSB + 4] * 4))
    x64 = x[:, :V].double().numpy()
    greedy = TR.timestamp_step(x64, [hist] * 4, [False] * 4, EOS, PAD, TSB, NOTS)[0] if rules else GR.greedy_step(x64, [False] * 4, EOS, PAD)[0]
    assert np.array_equal(tok, greedy), (tok, greedy)
    # ---- one allowed column: that column, log-prob 0
    one = TSB + 2 if rules else 17
    (tok, rows), got = run(hip, T.base_rows(2, 145), 0, 1.0, "one column", tables, hists=H([], []), ts_in=ts(-1, -1), sup=[c for c in ALL if c != one])
    assert tok.tolist() == [one, one] and (got["lp"] == 0.0).all()
    # ---- no allowed column: pad, 0, not finished
    kw = dict(bsup=[TSB], max_initial=0) if rules else dict(sup=ALL)
    (tok, rows), got = run(hip, T.base_rows(2, 146), 0, 1.0, "no column", tables, hists=H([], []), ts_in=ts(5, 6), **kw)
    assert tok.tolist() == [PAD, PAD] and (got["lp"] == 0.0).all() and got["n_unf"] == 2 and all(d["token"] is None for d in rows)


# ------------------------------------------------------------------------------------------------------------ 2. random rows
@pytest.mark.parametrize("path", ["vector", "ldv=127", "offset"])
def test_sample_step_random_rows(hip, path):
    """65 rows x V = 127 at T = 0.8, steps 0 .. 2, with and without the rules: the vector loop (128-column rows), and the scalar loop
    reached by ldv = 127 and by a logits pointer offset by one float.  The device token lies in the restatement's accept set
    (tests/test_whisper_sample_ref.py: none of these accept sets holds more than one column)."""
    R = SR.RANDOM_ROWS
    if path == "ldv=127":
        x = torch.from_numpy(SR.random_rows(SR.RANDOM_V)).to(DEV)
    else:
        x = torch.from_numpy(SR.random_rows(LDV)).to(DEV)
        if path == "offset":
            buf = torch.zeros(R * LDV + 1, dtype=torch.float32, device=DEV)
            buf[1:].view(R, LDV).copy_(x)
            x = buf[1:].view(R, LDV)
            assert x.data_ptr() % 16 == 4
    for t, hist in ((0, []), (1, [TSB + 3]), (2, [TSB + 3, 7])):
        for rules in (False, True):
            kw = dict(hists=[hist] * R, ts_in=[TR.last_timestamp(hist, TSB)] * R, max_initial=5) if rules else {}
            run(hip, x, t, SR.RANDOM_T, f"random {path} t={t} rules={rules}", seed=SR.RANDOM_SEED, planted=False, **kw)


# ------------------------------------------------------------------------------------------------------------ 3. the vocabulary's width
def test_sample_step_vocabulary_width(hip):
    """V = 51 866 in a 51 872-column buffer (ts_begin 50 365), 3 rows after [ts, text] at T = 1: the two-column tail behind the
    vector loop is drawn from like the rest (row 2's mass sits in the last column)."""
    Vw, ldv, tsb, nots, eos = 51866, 51872, 50365, 50364, 50257
    x = 3 * torch.randn(3, ldv, generator=torch.Generator().manual_seed(147))
    x[:, Vw:] = 1e30
    x[1, 1000] = 25.0
    x[2, Vw - 1] = 40.0
    hist = [tsb + 10, 500]
    (tok, rows), got = run(hip, x, 2, 1.0, f"V={Vw}", hists=[hist] * 3, ts_in=[tsb + 10] * 3, planted=False, Vn=Vw, eos=eos, pad=eos, tsb=tsb, nots=nots)
    assert tok[1] == 1000 and tok[2] == Vw - 1 and got["ts_last"].tolist() == [tok[0] if tok[0] >= tsb else tsb + 10, tsb + 10, Vw - 1]


# ------------------------------------------------------------------------------------------------------------ 4. determinism, independence
def test_sample_step_determinism_and_independence(hip, tables):
    x = torch.zeros(65, 8)
    kw = dict(Vn=8, eos=0, pad=0)
    a = launch(hip, x, 0, 1.0, SEED, **kw)
    b = launch(hip, x, 0, 1.0, SEED, **kw)
    assert np.array_equal(a["tok"], b["tok"]) and np.array_equal(a["lp_bits"], b["lp_bits"]), "the same call twice: the same bits"
    xr = T.base_rows(5, 148)
    hist = [[TSB + 4, 7]] * 5
    c = launch(hip, xr, 2, 0.9, SEED, tables, hists=hist, ts_in=[TSB + 4] * 5)
    d = launch(hip, xr, 2, 0.9, SEED, tables, hists=hist, ts_in=[TSB + 4] * 5)
    assert np.array_equal(c["tok"], d["tok"]) and np.array_equal(c["lp_bits"], d["lp_bits"]) and torch.equal(c["h_next"].view(torch.int16),
                                                                                                             d["h_next"].view(torch.int16))
    base = a["tok"][:64]
    other_seed = launch(hip, x, 0, 1.0, SEED + 1, **kw)["tok"][:64]
    other_t = launch(hip, x, 1, 1.0, SEED, **kw)["tok"][:64]
    other_row = a["tok"][1:65]
    changed = [int((base != o).sum()) for o in (other_seed, other_t, other_row)]
    print(f"flat 8-column row, 64 draws: another seed changes {changed[0]}, another t {changed[1]}, another row {changed[2]}")
    assert min(changed) >= 16
    assert np.array_equal(base, SR.sample_step(np.zeros((64, 8)), [False] * 64, 0, 0, 1.0, SEED, 0)[0])


# ------------------------------------------------------------------------------------------------------------ 5. the distribution
@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_sample_step_distribution_on_the_device(hip, temperature):
    """The 65 536 x 8 case of tests/test_whisper_sample_ref.py through the kernel (one launch, V = ldv = 8, step 3): the tokens equal the
    restatement's wherever its accept set is one column, and the device's own chi-square is below the same point."""
    x = SR.chi_logits()
    N = SR.CHI_N
    got = launch(hip, torch.from_numpy(np.tile(x, (N, 1))), 3, temperature, SR.CHI_SEED, Vn=8, eos=0, pad=0)
    want, single = SR.draw_rows(x, temperature, SR.CHI_SEED, 3, np.arange(N))
    chi, counts = SR.chi_square(got["tok"], x, temperature)
    differ = int((got["tok"] != want).sum())
    print(f"T = {temperature}: device chi-square {chi:.3f} (bar {SR.CHI2_7_999}), counts {counts.astype(int).tolist()}; {differ} tokens differ from "
          f"the restatement, {int((~single).sum())} accept sets hold more than one column")
    assert np.array_equal(got["tok"][single], want[single]) and chi < SR.CHI2_7_999
    lsm = GR.log_softmax(x.astype(np.float64)[None])[0]
    assert np.abs(got["lp"] - lsm[got["tok"]]).max() < 1e-5


# ------------------------------------------------------------------------------------------------------------ 6. refusals
def test_sample_step_refusals(hip, tables):
    E, Pz = tables
    R = 3
    x = T.base_rows(R, 149).to(DEV)
    tokens = torch.full((R, 3), -5, dtype=torch.int32, device=DEV)
    lps = torch.zeros((R, 3), dtype=torch.float32, device=DEV)
    fin = torch.zeros(R, dtype=torch.uint8, device=DEV)
    n_unf = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    ts_last = torch.full((R,), 55, dtype=torch.int32, device=DEV)
    h_next = torch.full((R, De), 7.0, dtype=torch.bfloat16, device=DEV)
    kw = dict(finished=fin, n_unfinished=n_unf, tokens=tokens, logprobs=lps, embed_tokens=E.to(DEV), embed_positions=Pz.to(DEV), h_next=h_next)
    ok = dict(t=0, eos_id=EOS, pad_id=PAD, ts_begin=TSB, no_timestamps_id=NOTS, ts_last=ts_last, next_pos=0, temperature=1.0, seed=1)
    for change, match in ((dict(temperature=0.0), "temperature"), (dict(temperature=-0.5), "temperature"), (dict(temperature=float("nan")), "temperature"),
                          (dict(temperature=1e-45), "temperature"), (dict(temperature=0.0, ts_last=None), "temperature"),
                          (dict(eos_id=V), "eos_id"), (dict(pad_id=-1), "pad_id"), (dict(t=3), "step t"), (dict(next_pos=MAXP), "overruns"),
                          (dict(eos_id=V, ts_last=None), "eos_id"), (dict(ts_begin=EOS), "ts_begin"), (dict(ts_begin=V), "ts_begin"),
                          (dict(no_timestamps_id=V), "no_timestamps_id")):
        with pytest.raises(ValueError, match=match):
            hip.dec_sample_step(x, V, **dict(ok, **change), **kw)
    torch.cuda.synchronize()
    assert bool((tokens == -5).all()) and int(n_unf.item()) == 77 and bool((h_next == 7.0).all()) and bool((ts_last == 55).all()) \
        and bool((fin == 0).all()), "a refused call launched"


# ------------------------------------------------------------------------------------------------------------ 7. generate
@pytest.mark.parametrize("timestamps", [False, True])
def test_generate_sampling_best_of(model, enc, golden, timestamps):
    from ssak_amd.whisper_seq2seq import beam_rank, sample_call_seed
    enc_lens = golden["enc_lens"]
    prompt, sup, rules = SR.gen_case(golden, timestamps)
    n, B = SR.GEN_N, 3
    call = lambda **kw: model.generate(enc, enc_lens=enc_lens, language=SR.GEN_LANGS, suppress_tokens=sup, max_new_tokens=SR.GEN_NEW,
                                       timestamps=timestamps, **kw)
    r = call(temperature=SR.GEN_T, best_of=n, seed=SR.GEN_SEED)
    print(f"generate(T={SR.GEN_T}, best_of={n}, timestamps={timestamps}): samples {[[c[0] for c in s] for s in r.samples]}")
    assert len(r.samples) == B and all(len(s) == n for s in r.samples) and r.beams is None
    assert (r.no_speech_prob is not None and r.no_speech_prob.shape == (B,)) if timestamps else r.no_speech_prob is None
    # teacher-forced: the float64 rule with the same noise on the project's own logits of the device's history
    rows = [c[0] for s in r.samples for c in s]
    width = max(len(k) for k in rows)
    P = prompt.shape[1]
    full = np.full((B * n, P + width), G.EOT, dtype=np.int64)
    full[:, :P] = np.repeat(prompt, n, axis=0)
    for k, toks in enumerate(rows):
        full[k, P:P + len(toks)] = toks
    logits = model.decode_logits(enc.repeat_interleave(n, dim=0), full, np.repeat(enc_lens, n)).double().cpu().numpy()
    kseed = sample_call_seed(SR.GEN_SEED)
    steps = excused = 0
    for k, toks in enumerate(rows):
        for i, tok in enumerate(toks):
            _, _, _, ds = SR.sample_step(logits[k:k + 1, P - 1 + i], [False], G.EOT, G.EOT, SR.GEN_T, kseed, i, [list(toks[:i])] if timestamps else None,
                                         suppress=sup, row0=k, **(rules or dict()))
            steps += 1
            if ds[0]["gap"] < SR.GEN_BAR:
                excused += 1
                continue
            assert tok == ds[0]["token"], (k, i, tok, ds[0]["token"], ds[0]["gap"])
        if timestamps:
            TR.check_grammar(list(toks), TSB, EOS, NOTS, T.MAX_INITIAL)
        assert not np.isin(toks, sup).any()
    print(f"teacher-forced: {excused} of {steps} steps below the score gap {SR.GEN_BAR:.4f} (excused; at most a quarter)")
    assert excused <= steps / 4
    # ranking, and the chosen candidate in the existing fields
    for b in range(B):
        cands = [(toks, s, bool(toks) and toks[-1] == G.EOT, j) for j, (toks, s) in enumerate(r.samples[b])]
        w = beam_rank(cands)
        assert r.tokens[b] == cands[w][0] and r.sum_logprob[b] == cands[w][1] and r.lens[b] == len(cands[w][0])
        assert np.array_equal(r.logprobs[b, :r.lens[b]], r.sample_logprobs[b][w]) and r.avg_logprob[b] == r.sum_logprob[b] / (r.lens[b] + 1)
        assert all(abs(lp.sum() - s) < 1e-12 and len(lp) == len(toks) for lp, (toks, s) in zip(r.sample_logprobs[b], r.samples[b]))
        assert len({tuple(c[0]) for c in r.samples[b]}) > 1, "the candidates of an audio differ by their row"
    # the same seed, another seed, best_of = None
    again = call(temperature=SR.GEN_T, best_of=n, seed=SR.GEN_SEED)
    assert again.samples == r.samples and again.tokens == r.tokens and np.array_equal(again.logprobs, r.logprobs)
    assert call(temperature=SR.GEN_T, best_of=n, seed=SR.GEN_SEED + 1).samples != r.samples
    one = call(temperature=SR.GEN_T, seed=SR.GEN_SEED)
    assert all(len(s) == 1 for s in one.samples) and one.tokens == [s[0][0] for s in one.samples]
    # temperature 0: what the call returned before, best_of and seed ignored
    plain, zero = call(), call(temperature=0.0, best_of=n, seed=5)
    assert zero.tokens == plain.tokens and np.array_equal(zero.logprobs, plain.logprobs) and zero.samples is None and plain.samples is None
    for bad, match in ((dict(temperature=0.5, beam_size=2), "beam_size"), (dict(temperature=0.5, best_of=9), "best_of"),
                       (dict(temperature=0.5, best_of=0), "best_of"), (dict(temperature=-1.0), "temperature"), (dict(temperature=float("nan")), "temperature")):
        with pytest.raises(ValueError, match=match):
            call(**bad)


# ------------------------------------------------------------------------------------------------------------ 8. transcribe
def test_transcribe_temperature_fallback(long_model, noise):
    """Two files of 35 s and 31 s (two windows each) on the long-form tiny model.  Its random weights give average log-probabilities
    far below -1, so the default thresholds drive every window through the temperatures.  In the last case every id maps to the same
    letters ("a" x 16 per id, one run for a window without text: zlib's fixed cost keeps 16 single letters below 2.4)."""
    m = long_model
    files = [noise[2][:35 * 16000], noise[1]]
    calls = []
    gen = m.generate

    def counting(enc_out, **kw):
        calls.append((enc_out.shape[0], kw.get("temperature", 0.0), kw.get("best_of"), kw.get("beam_size"), kw.get("seed")))
        return gen(enc_out, **kw)

    encodes = []
    encode = m.encode
    m.generate, m.encode = counting, lambda f: encodes.append(f.shape[0]) or encode(f)
    try:
        res = m.transcribe(files, temperature=(0.0, 0.4, 0.8), best_of=2, beam_size=2, _max_rounds=16)
        n_calls, n_enc = len(calls), len(encodes)
        off = m.transcribe(files, temperature=(0.0, 0.4, 0.8), best_of=2, compression_ratio_threshold=None, logprob_threshold=None,
                           no_speech_threshold=None, _max_rounds=16)
        base = m.transcribe(files, logprob_threshold=None, no_speech_threshold=None, _max_rounds=16)
        text_of = lambda ids: "a" * (16 * max(len(ids), 1))
        ratio = m.transcribe(files, temperature=(0.0, 0.4, 0.8), best_of=2, logprob_threshold=-1e9, text_of=text_of, _max_rounds=16)
        same = m.transcribe(files, temperature=(0.0, 0.4, 0.8), best_of=2, beam_size=2, _max_rounds=16)
    finally:
        del m.generate, m.encode
    print(f"fallback: generate calls (rows, T, best_of, beam, seed) {calls[:n_calls]}; encoder calls {encodes[:n_enc]}; avg_logprob "
          f"{[[round(w.avg_logprob, 2) for w in r.windows] for r in res]}; no_speech_prob {[[round(w.no_speech_prob, 4) for w in r.windows] for r in res]}")
    for r in res:
        assert len(r.windows) >= 2 and all(w.temperature == 0.8 and w.avg_logprob < -1.0 for w in r.windows)
        for w in r.windows:
            TR.check_grammar(w.tokens, NOTS + 1, EOS, NOTS, 50)
    per_round = [calls[:n_calls][i:i + 3] for i in range(0, n_calls, 3)]
    assert n_calls % 3 == 0 and n_calls >= 6 and all([c[1] for c in rnd] == [0.0, 0.4, 0.8] for rnd in per_round)
    assert n_enc == n_calls // 3, "one encoder call per round: a retry reads the round's encoder output again"
    assert all(rnd[0][0] == rnd[1][0] == rnd[2][0] for rnd in per_round), "every window of a round fails: the whole round is decoded again"
    assert all(rnd[0][2:4] == (None, 2) and rnd[1][2:4] == (2, None) for rnd in per_round), "temperature 0 takes the beam, above 0 best_of"
    assert len({c[4] for c in calls[:n_calls] if c[1] > 0}) == 2 * n_calls // 3, "every sampling call draws with its own seed"
    assert [[w.tokens for w in r.windows] for r in same] == [[w.tokens for w in r.windows] for r in res] and \
        [r.segments for r in same] == [r.segments for r in res], "the same seed: the same result"
    for r, b in zip(off, base):
        assert all(w.temperature == 0.0 and w.compression_ratio == 0.0 for w in r.windows)
        assert r.segments == b.segments and r.seeks == b.seeks and [w.tokens for w in r.windows] == [w.tokens for w in b.windows]
    print(f"compression ratio alone: {[[round(w.compression_ratio, 2) for w in r.windows] for r in ratio]}")
    for r in ratio:
        assert all(w.temperature == 0.8 and w.compression_ratio > 2.4 for w in r.windows)


# ------------------------------------------------------------------------------------------------------------ 9. the command line
def test_command_line_accurate(long_weights, noise, tmp_path, capsys):
    from ssak_amd import whisper_infer
    folder = G.write_folder(T._Stored(long_weights, T.long_generation_config()), str(tmp_path / "model"), max_source_positions=1500,
                            encoder_layers=1, config_overrides={"vocab_size": T.VT})
    path = str(tmp_path / "noise31.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1), f.setsampwidth(2), f.setframerate(16000)
        f.writeframes((noise[1].numpy() * 32767).astype("<i2").tobytes())
    outs = []
    for _ in range(2):
        whisper_infer.main([path, "--model", folder, "--language", "en", "--timestamps", "--accurate", "--seed", "7"])
        cap = capsys.readouterr()
        outs.append(cap.out.strip().splitlines())
    print(f"--timestamps --accurate --seed 7: {len(outs[0])} lines, first {outs[0][:1]}; stderr {cap.err.strip()!r}")
    assert len(outs[0]) >= 1 and outs[0] == outs[1], "the same command prints the same lines"
    assert "compression-ratio check" in cap.err, "no tokenizer in the folder: one line on stderr"
    for line in outs[0]:
        p, a, b, ids = line.split("\t")[:4]
        assert p == path and 0.0 <= float(a) < float(b) <= 31.0 + 30.0 and all(0 <= int(t) < NOTS + 1 for t in ids.split())
    with pytest.raises(SystemExit):
        whisper_infer.main([path, "--model", folder, "--language", "en", "--accurate"])
    capsys.readouterr()
