"""GPU: utterance classification (ssak_amd/csrc/classify.hip, ssak_amd/classify.py) against the float64 restatement
tests/classify_ref.py and the golden of tests/gen_golden_classify.py (transformers.HubertModel + the restated head, fp32).

Per-op bars come from the roundings, not from what the kernels return.  With u = 2^-24 (fp32 unit roundoff) a sum of K fp32
terms accumulated in fp32, in ANY order, is within K u sum|terms| of the exact sum; a value stored as bf16 is within half a
bf16 ulp <= 2^-8 |value| of what was stored.  Every reference is computed in float64 from EXACTLY the values the kernel is given
(bf16 hidden states, fp32 weights and gradients, the device's own dropout bits), so these are the only error sources:

  pool sum    K = len terms                                      bar = K u sum_f |h|
  pool mean   the same, then one division                        bar = (K + 1) u sum_f |h| / len
  pool max    a selection: no arithmetic                         bar = 0, argmax identical (the reference's maximum is unique)
  pool bwd    a copy (sum, max) or one fp32 division (mean),     bar = (2^-8 + 2 u) |ref| for bf16, 2 u |ref| for fp32
              then the store
  head z      K = H products + bias, one more rounding for       bar_z = (H + 2) u (sum_k |xd w1| + |b1|)
              the dropout scale
  head act    tanh is 1-Lipschitz; tanhf within 2 ulp, |a| <= 1  bar_a = bar_z + 4 u
  logits      K = H products + bias + scale, and the error of    bar_l = (H + 2) u (sum_k |ad w2| + |b2|) + sum_k |w2| m2 bar_a
              act carried through
  head bwd    (reference from the fp32 x, act, dlogits the kernel reads)
    dW2, db2  K = B terms (+ scale)                              (B + 1) u sum_b |g ad|;  B u sum_b |g|
    dz        K = C terms, then * m2 * (1 - a^2): the factor     bar_dz = (C + 5) u m2 sum_c |g w2|
              1 - a^2 is within 2 u, two more products
    dW1, db1  K = B terms (+ scale) + the error of dz carried    (B + 1) u sum_b |dz xd| + sum_b bar_dz |xd|;  B u sum_b |dz| + sum_b bar_dz
    dpooled   K = H terms (+ scale) + the error of dz carried    (H + 1) u m1 sum_j |dz w1| + m1 sum_j bar_dz |w1|
  softmax     with D = max_c |l_c - max l|: the exponent's rounding costs D 2u per exp, expf 1 ulp = 2u, both in numerator
              and denominator; C terms in the denominator, one division:  bar_p = (4 D + C + 6) u p
  loss        per utterance log(sum) + m - l_label: the denominator's relative error, logf 1 ulp, two additions; then the
              mean over B:  bar = mean_b[(4 D + C + 6) u + 2 u (|log s| + |m| + |l_label| + |nll|)] + (B + 1) u mean_b |nll|
  dlogits     (p - onehot) * (grad_scale / B): bar_p scaled, plus three roundings:  bar_p gs / B + 3 u |ref|

Pooling runs at two shapes (POOL_SHAPES below): one that stays in the forward kernel's one-frame tail loop and one whose
lengths cross its four-frame loop.

End to end (golden folder -> load_classifier) the project's existing bars hold: fp32-exact mode logits within 2e-4 and every
gradient tensor within 5e-3 of its largest element; bf16 engine logits 2e-2 and gradients 6e-2 in relative L2.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import classify_ref as R  # noqa: E402
import gen_golden_classify as G  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
HALF_BF16_ULP = 2.0 ** -8
B, H = 3, 72  # H: 9 chunks of 8 columns, no multiple of 64
# Pooling shapes: name -> (F, lens, seed).  The forward gives the frames r, r + 16, ... to frame group r, four at a time while
# f + 48 < len and one at a time after that, so a thread enters the four-frame loop only from len = 49 on:
#   F37   every thread stays in the one-frame tail (up to three rounds of it); a length of 1
#   F131  len 131: two rounds of the four-frame loop, then a tail for the groups 0..2 only; len 49: the loop once for group 0
#         alone; len 64 (a multiple of the 64 frames of a round): the loop exactly once for every group and no tail
# Each seed gives bf16 hidden states with a unique maximum per (utterance, column), with and without lengths (asserted).
POOL_SHAPES = {"F37": (37, (37, 1, 20), 10), "F131": (131, (131, 49, 64), 71)}
F, LENS = POOL_SHAPES["F37"][:2]  # the shape the argument-error test uses
MODES = ("mean", "sum", "max")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    import ssak_amd.hip as h
    return h


@pytest.fixture(scope="module")
def pool_cases():
    """Per shape: hidden [B, F, H] as bf16 values (exact in float64), dpooled as fp32 values, the float64 references of every
    mode with and without lengths.  Computed once, read by every pooling test."""
    cases = {}
    for name, (frames, lens_, seed) in POOL_SHAPES.items():
        g = torch.Generator().manual_seed(seed)
        hidden = torch.randn(B, frames, H, generator=g).bfloat16()
        dpooled = torch.randn(B, H, generator=g)
        h64 = hidden.double().numpy()
        ref = {}
        for lens in (None, lens_):
            for mode in MODES:
                pooled, argmax = R.pool_fwd(h64, lens, mode)
                ref[(lens, mode)] = dict(pooled=pooled, argmax=argmax, abs_sum=R.pool_abs_sum(h64, lens),
                                         dhidden=R.pool_bwd(dpooled.double().numpy(), frames, lens, mode, argmax))
        cases[name] = (hidden, dpooled, h64, ref)
    return cases


@pytest.fixture(scope="module")
def pool_case(pool_cases):
    return pool_cases["F37"]


def _unique_max(h64, lens):
    for b in range(B):
        v = h64[b, :(h64.shape[1] if lens is None else lens[b])]
        if ((v == v.max(0)).sum(0) != 1).any():
            return False
    return True


@pytest.mark.parametrize("with_lens", [False, True], ids=["all", "lens"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(POOL_SHAPES))
def test_pool_fwd(hip, pool_cases, shape, mode, with_lens):
    hidden, _, h64, ref = pool_cases[shape]
    frames = POOL_SHAPES[shape][0]
    lens = POOL_SHAPES[shape][1] if with_lens else None
    r = ref[(lens, mode)]
    if mode == "max":
        assert _unique_max(h64, lens), "pick another seed: the reference's maximum must be unique"
    for dtype in (torch.bfloat16, torch.float32):  # the engine's storage type and the fp32-exact mode's, same values
        pooled, argmax = hip.pool_fwd(hidden.to(DEV, dtype), lens, mode)
        n = np.full(B, frames) if lens is None else np.asarray(lens)
        if mode == "sum":
            bar = n[:, None] * U * r["abs_sum"]
        elif mode == "mean":
            bar = (n[:, None] + 1) * U * r["abs_sum"] / n[:, None]
        else:
            bar = np.zeros((B, H))
            assert np.array_equal(argmax.cpu().numpy(), r["argmax"])
        err = np.abs(pooled.cpu().double().numpy() - r["pooled"])
        print(f"pool_fwd {shape} {mode} lens={lens} {dtype}: max err {err.max():.3e}, min bar {bar.min():.3e}")
        assert (err <= bar).all(), (shape, mode, lens, dtype, float((err - bar).max()))
        assert (argmax is None) == (mode != "max")


@pytest.mark.parametrize("with_lens", [False, True], ids=["all", "lens"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(POOL_SHAPES))
def test_pool_bwd(hip, pool_cases, shape, mode, with_lens):
    _, dpooled, _, ref = pool_cases[shape]
    frames = POOL_SHAPES[shape][0]
    lens = POOL_SHAPES[shape][1] if with_lens else None
    r = ref[(lens, mode)]
    argmax = None if mode != "max" else torch.tensor(r["argmax"], dtype=torch.int32, device=DEV)
    for dtype, store in ((torch.bfloat16, HALF_BF16_ULP), (torch.float32, 0.0)):
        d = hip.pool_bwd(dpooled.to(DEV), argmax, lens, frames, mode, dtype)
        assert d.shape == (B, frames, H) and d.dtype == dtype
        got = d.cpu().double().numpy()
        bar = (store + 2 * U) * np.abs(r["dhidden"])
        err = np.abs(got - r["dhidden"])
        print(f"pool_bwd {shape} {mode} lens={lens} {dtype}: max err {err.max():.3e}")
        assert (err <= bar).all(), (shape, mode, lens, dtype)
        assert (got[r["dhidden"] == 0] == 0).all()  # beyond len and off the argmax frame: exact zeros, every element written
        if lens is not None:
            for b in range(B):
                assert (got[b, lens[b]:] == 0).all()
        if mode != "mean":  # no arithmetic: the stored value is the bf16 rounding of the reference
            assert torch.equal(d.cpu(), torch.tensor(r["dhidden"]).to(dtype))


def _head_case(C, seed=11):
    g = torch.Generator().manual_seed(seed + C)
    x = torch.randn(B, H, generator=g)
    W1, b1 = torch.randn(H, H, generator=g) / H ** 0.5, 0.1 * torch.randn(H, generator=g)
    W2, b2 = torch.randn(C, H, generator=g) / H ** 0.5, 0.1 * torch.randn(C, generator=g)
    dlogits = torch.randn(B, C, generator=g)
    return x, W1, b1, W2, b2, dlogits


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("C", [2, 5])
def test_head_fwd_bwd(hip, C, p):
    x, W1, b1, W2, b2, dlogits = _head_case(C)
    seed, training = 0x1234_5678_9ABC, p > 0
    m1 = m2 = None
    if p > 0:  # the device's own bits of the two sites, with the factor the kernels multiply kept elements by
        k1, s1 = hip.debug_dropout_mask(seed, hip.CLS_SITE_INPUT, p, B, H, DEV)
        k2, s2 = hip.debug_dropout_mask(seed, hip.CLS_SITE_HIDDEN, p, B, H, DEV)
        m1, m2 = k1.cpu().double().numpy() * s1, k2.cpu().double().numpy() * s2
        assert 0.1 < 1 - k1.float().mean().item() < 0.4 and not torch.equal(k1, k2)
    d = [t.to(DEV) for t in (x, W1, b1, W2, b2)]
    logits, act = hip.cls_head_fwd(*d, drop_p=p, seed=seed, training=training)
    x64, W164, b164, W264, b264 = (t.double().numpy() for t in (x, W1, b1, W2, b2))
    f = R.head_fwd(x64, W164, b164, W264, b264, m1, m2)
    one = np.ones((B, H))
    mm1, mm2 = (one if m1 is None else m1), (one if m2 is None else m2)
    bar_z = (H + 2) * U * (np.abs(f["xd"]) @ np.abs(W164).T + np.abs(b164))
    bar_a = bar_z + 4 * U
    bar_l = (H + 2) * U * (np.abs(f["ad"]) @ np.abs(W264).T + np.abs(b264)) + (mm2 * bar_a) @ np.abs(W264).T
    e_a, e_l = np.abs(act.cpu().double().numpy() - f["a"]), np.abs(logits.cpu().double().numpy() - f["logits"])
    print(f"head fwd C={C} p={p}: act err {e_a.max():.3e} (bar >= {bar_a.min():.3e}), logits err {e_l.max():.3e} (bar >= {bar_l.min():.3e})")
    assert (e_a <= bar_a).all() and (e_l <= bar_l).all()
    if p > 0:  # training = 0 turns the dropout off whatever p says
        lg0, _ = hip.cls_head_fwd(*d, drop_p=p, seed=seed, training=False)
        lg1, _ = hip.cls_head_fwd(*d, drop_p=0.0, seed=seed, training=True)
        assert torch.equal(lg0, lg1) and not torch.equal(lg0, logits)

    # backward: the reference reads the fp32 act the kernel reads
    a64 = act.cpu().double().numpy()
    fb = dict(a=a64, ad=a64 * mm2, xd=x64 * mm1)
    g64 = dlogits.double().numpy()
    r = R.head_bwd(g64, x64, W164, W264, fb, m1, m2)
    nan = float("nan")
    dW1, db1 = torch.full((H, H), nan, device=DEV), torch.full((H,), nan, device=DEV)
    dW2, db2 = torch.full((C, H), nan, device=DEV), torch.full((C,), nan, device=DEV)
    dx = hip.cls_head_bwd(dlogits.to(DEV), d[0], act, d[1], d[3], dW1, db1, dW2, db2, drop_p=p, seed=seed, training=training)
    ag = np.abs(g64)
    bar_dz = (C + 5) * U * mm2 * (ag @ np.abs(W264))
    adz, axd = np.abs(r["dz"]), np.abs(fb["xd"])
    bars = dict(dW2=(B + 1) * U * (ag.T @ np.abs(fb["ad"])), db2=B * U * ag.sum(0),
                dW1=(B + 1) * U * (adz.T @ axd) + bar_dz.T @ axd, db1=B * U * adz.sum(0) + bar_dz.sum(0),
                dx=(H + 1) * U * mm1 * (adz @ np.abs(W164)) + mm1 * (bar_dz @ np.abs(W164)))
    for name, got in (("dW1", dW1), ("db1", db1), ("dW2", dW2), ("db2", db2), ("dx", dx)):
        err = np.abs(got.cpu().double().numpy() - r[name])
        print(f"head bwd C={C} p={p} {name}: max err {err.max():.3e}, max bar {bars[name].max():.3e}")
        assert (err <= bars[name]).all(), name
        if m1 is not None and name == "dx":
            assert (got.cpu().numpy()[m1 == 0] == 0).all()


@pytest.mark.parametrize("C", [2, 5])
def test_softmax_ce(hip, C):
    g = torch.Generator().manual_seed(5 + C)
    logits = 3 * torch.randn(B, C, generator=g)
    labels = [C - 1, 0, 1]
    gs = 0.5
    probs, loss, dl = hip.cls_softmax_ce(logits.to(DEV), labels, gs)
    l64 = logits.double().numpy()
    p, rloss, rdl = R.softmax_ce(l64, labels, gs)
    m = l64.max(1)
    D = np.abs(l64 - m[:, None]).max(1)
    rel = (4 * D + C + 6) * U
    bar_p = rel[:, None] * p
    s = np.exp(l64 - m[:, None]).sum(1)
    nll = -np.log(p[np.arange(B), labels])
    bar_loss = (rel + 2 * U * (np.abs(np.log(s)) + np.abs(m) + np.abs(l64[np.arange(B), labels]) + nll)).mean() + (B + 1) * U * nll.mean()
    bar_dl = bar_p * gs / B + 3 * U * np.abs(rdl)
    e_p = np.abs(probs.cpu().double().numpy() - p)
    e_loss = abs(loss.item() - rloss)
    e_dl = np.abs(dl.cpu().double().numpy() - rdl)
    print(f"softmax_ce C={C}: probs err {e_p.max():.3e}, loss err {e_loss:.3e} (bar {bar_loss:.3e}), dlogits err {e_dl.max():.3e}")
    assert (e_p <= bar_p).all() and e_loss <= bar_loss and (e_dl <= bar_dl).all()
    probs2, loss2, dl2 = hip.cls_softmax_ce(logits.to(DEV))  # prediction: no labels, no loss
    assert loss2 is None and dl2 is None and torch.equal(probs2, probs)


def test_bad_arguments_are_errors_not_faults(hip, pool_case):
    hidden, dpooled, _, ref = pool_case
    hd = hidden.to(DEV)
    with pytest.raises(ValueError, match="frame_lens"):
        hip.pool_fwd(hd, (37, 0, 20), "mean")  # len = 0
    with pytest.raises(ValueError, match="frame_lens"):
        hip.pool_fwd(hd, (37, 38, 20), "mean")  # len > F
    with pytest.raises(ValueError, match="frame_lens"):
        hip.pool_bwd(dpooled.to(DEV), None, (37, 0, 20), F, "mean")
    with pytest.raises(ValueError, match="multiple of 8"):
        hip.pool_fwd(torch.zeros(B, F, 76, dtype=torch.bfloat16, device=DEV), None, "sum")  # H % 8 != 0
    with pytest.raises(ValueError, match="multiple of 8"):
        hip.pool_bwd(torch.zeros(B, 76, device=DEV), None, None, F, "sum")
    logits = torch.zeros(B, 2, device=DEV)
    for bad in ((0, 2, 1), (0, -1, 1)):
        with pytest.raises(ValueError, match="label"):
            hip.cls_softmax_ce(logits, bad)
    with pytest.raises(ValueError, match="multiple of 4"):
        hip.cls_head_fwd(torch.zeros(B, 6, device=DEV), torch.zeros(6, 6, device=DEV), torch.zeros(6, device=DEV),
                         torch.zeros(2, 6, device=DEV), torch.zeros(2, device=DEV))
    # nothing was launched and nothing is poisoned: the same buffers still pool
    pooled, _ = hip.pool_fwd(hd, LENS, "sum")
    assert np.abs(pooled.cpu().double().numpy() - ref[(LENS, "sum")]["pooled"]).max() < 1e-4


# ------------------------------------------------------------------------------------------------ end to end: the golden folder
@pytest.fixture(scope="module")
def golden(gold, tmp_path_factory):
    z = gold("classify_tiny.npz")
    return z, G.write_folder(z, str(tmp_path_factory.mktemp("classify_tiny")))


def _ref_grads(z):
    return {k[2:].replace("hubert.", "wav2vec2.", 1): z[k] for k in z.files if k.startswith("g/")}


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / (np.sqrt((b ** 2).sum()) + 1e-12))


def test_golden_folder_exact_mode(golden):
    """fp32-exact engine: logits within 2e-4, loss 1e-4, every stored gradient tensor within 5e-3 of its largest element."""
    from ssak_amd.classify import load_classifier
    z, folder = golden
    model = load_classifier(folder, exact=True).train()
    assert model.config.model_type == "hubert" and model.config.pooling_mode == "mean" and model.config.id2label == {0: "F", 1: "M"}
    out = model(torch.tensor(z["x"]), labels=z["labels"])
    e_logits = float(np.abs(out.logits.cpu().numpy() - z["logits"]).max())
    e_loss = abs(out.loss.item() - float(z["loss"])) / float(z["loss"])
    assert np.abs(out.probs.cpu().numpy() - z["probs"]).max() < 2e-4
    model.head_grads.fill_(float("nan"))
    model.encoder.grads[:model.encoder.num_trainable].fill_(float("nan"))
    model.backward()
    ref = _ref_grads(z)
    floor = 1e-3 * max(float(np.abs(g).max()) for g in ref.values())
    worst = ("", 0.0)
    for n, g in ref.items():
        e = float(np.abs(model.grad(n).cpu().numpy() - g).max()) / max(float(np.abs(g).max()), floor)
        worst = max(worst, (n, e), key=lambda t: t[1])
    print("classify exact: logits max abs err", e_logits, "loss rel err", e_loss, "worst grad", worst)
    assert e_logits < 2e-4 and e_loss < 1e-4 and worst[1] < 5e-3
    assert not torch.isnan(model.encoder.grads[:model.encoder.num_trainable]).any()
    assert float(model.encoder.grad("lm_head.weight").abs().max()) == 0.0  # the unused CTC head


def test_exact_mode_hidden_state(golden):
    """forward_hidden in the fp32-exact mode hands over a float hidden state: held directly to the golden's last_hidden_state,
    within the exact mode's 2e-4 of the largest element."""
    from ssak_amd.classify import load_classifier
    z, folder = golden
    hidden, _ = load_classifier(folder, exact=True).encoder.forward_hidden(torch.tensor(z["x"]))
    assert hidden.dtype == torch.float32 and tuple(hidden.shape) == z["hidden"].shape
    e = float(np.abs(hidden.cpu().numpy() - z["hidden"]).max() / np.abs(z["hidden"]).max())
    print("classify exact: hidden state max err / max", e)
    assert e < 2e-4


def test_golden_folder_bf16_engine(golden, tmp_path):
    """The production engine: logits and loss within 2e-2, gradients within 6e-2 (relative L2); eval-mode logits identical;
    save_classifier writes the HuBERT names back."""
    from ssak_amd.classify import load_classifier, save_classifier
    z, folder = golden
    model = load_classifier(folder).train()
    out = model(torch.tensor(z["x"]), labels=z["labels"])
    e_logits = rel_l2(out.logits.cpu().numpy(), z["logits"])
    e_loss = abs(out.loss.item() - float(z["loss"])) / float(z["loss"])
    model.head_grads.fill_(float("nan"))
    model.backward()
    ref = _ref_grads(z)
    gmax = max(float(np.abs(g).max()) for g in ref.values())
    worst = ("", 0.0)
    for n, g in ref.items():
        got = model.grad(n).cpu().numpy()
        if np.abs(g).max() < 2e-4 * gmax:  # numerically-zero gradients (k_proj.bias): absolute check
            assert np.abs(got - g).max() < 1e-3 * gmax, n
            continue
        worst = max(worst, (n, rel_l2(got, g)), key=lambda t: t[1])
    print("classify bf16: logits rel err", e_logits, "loss rel err", e_loss, "worst grad", worst)
    assert e_logits < 2e-2 and e_loss < 2e-2 and worst[1] < 6e-2
    with pytest.raises(RuntimeError):
        model.backward()  # consumed
    out2 = model.eval()(torch.tensor(z["x"]))
    assert out2.loss is None and torch.equal(out2.logits, out.logits)  # every regulariser of the golden configuration is off
    save_classifier(model, str(tmp_path))
    from safetensors.torch import load_file
    sd = load_file(os.path.join(str(tmp_path), "model.safetensors"))
    stored = {k[2:] for k in z.files if k.startswith("w/")}
    assert stored <= set(sd) and all(k.startswith(("hubert.", "classifier.")) for k in sd)
    assert all(np.array_equal(sd[k].numpy(), z["w/" + k]) for k in stored)
    with open(os.path.join(str(tmp_path), "config.json")) as f:
        assert json.load(f)["model_type"] == "hubert"


def test_load_classifier_refuses_other_hubert_graphs(golden, tmp_path):
    from ssak_amd.classify import SpeechClassifier, SpeechClassifierConfig, load_classifier
    z, folder = golden
    cfg = json.loads(str(z["config_json"]))
    for field, value in (("feat_proj_layer_norm", False), ("conv_pos_batch_norm", True)):
        d = tmp_path / field
        d.mkdir()
        (d / "config.json").write_text(json.dumps(dict(cfg, **{field: value})))
        os.symlink(os.path.join(folder, "model.safetensors"), d / "model.safetensors")
        with pytest.raises(ValueError, match=field):
            load_classifier(str(d))
    for kw in (dict(problem_type="regression"), dict(problem_type="multi_label_classification"), dict(num_labels=1)):
        with pytest.raises(NotImplementedError):
            SpeechClassifier(SpeechClassifierConfig(**kw))


def test_predict_gender(golden):
    from ssak_amd.classify import predict_gender
    z, folder = golden
    want = {0: "f", 1: "m"}[int(np.argmax(z["probs"][0]))]
    assert predict_gender(z["wave"][0], model=folder) == want
    scores = predict_gender(z["wave"][0], 16000, DEV, folder, "scores")
    assert set(scores) == {"m", "f"} and abs(sum(scores.values()) - 1) < 1e-6
    assert abs(scores["f"] - float(z["probs"][0][0])) < 2e-2 and max(scores, key=scores.get) == want
    # another sample rate goes through the resampler: the same speaker at 8 kHz still gives two scores that sum to 1
    s8 = predict_gender(z["wave"][0][::2].copy(), sample_rate=8000, model=folder, output_type="scores")
    assert set(s8) == {"m", "f"} and abs(sum(s8.values()) - 1) < 1e-6
    with pytest.raises(ValueError):
        predict_gender(z["wave"][0], model=folder, output_type="nope")
    with pytest.raises(FileNotFoundError):
        predict_gender(z["wave"][0], model=os.path.join(folder, "missing"))


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_classifier_with_lengths_dropout_and_grad_scale(golden, tmp_path, hip, mode):
    """SpeechClassifier end to end on the paths the golden run does not take: sample lengths (the valid frames only are pooled and
    the frame lengths reach the pooling backward), head dropout 0.25 under the step's seed, and backward(grad_scale = 0.5).  The
    reference is tests/classify_ref.py run on the bf16 hidden state the encoder returns for the same input and on the device's
    own dropout bits, so only fp32 roundings separate the two: at most six chained fp32 sums of at most H = 64 terms,
    6 * 65 * 2^-24 = 2.3e-5 of sum|terms|; with sum|terms| allowed ten times a tensor's largest element the bar is 2.4e-4 of that
    element (2^-12), plus half a bf16 ulp (2^-8, relative, per element) for d hidden, which is stored as bf16.  A wiring mistake
    (lengths, masks, seed, scale) moves these by their own size."""
    from ssak_amd.classify import load_classifier
    z, folder = golden
    cfg = dict(json.loads(str(z["config_json"])), pooling_mode=mode, final_dropout=0.25)
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    os.symlink(os.path.join(folder, "model.safetensors"), tmp_path / "model.safetensors")
    model = load_classifier(str(tmp_path)).train()
    assert model.config.pooling_mode == mode and model.config.final_dropout == 0.25
    x, labels, lengths, gs = torch.tensor(z["x"]), [0, 1], np.array([8000, 5000]), 0.5
    hidden, flens = model.encoder.forward_hidden(x, lengths=lengths)  # every regulariser of the encoder is off: the same again below
    frame_lens = flens.cpu().numpy()
    Bn, Fn, Hn = hidden.shape
    assert frame_lens[0] == Fn and 1 <= frame_lens[1] < Fn

    out = model(x, lengths=lengths, labels=labels)
    seed, p = model.encoder._used_seed, 0.25
    k1, s1 = hip.debug_dropout_mask(seed, hip.CLS_SITE_INPUT, p, Bn, Hn, DEV)
    k2, s2 = hip.debug_dropout_mask(seed, hip.CLS_SITE_HIDDEN, p, Bn, Hn, DEV)
    assert 0 < int(k1.sum()) < Bn * Hn and 0 < int(k2.sum()) < Bn * Hn
    W = [model.head_param(n).cpu().double().numpy() for n in ("classifier.dense.weight", "classifier.dense.bias",
                                                              "classifier.out_proj.weight", "classifier.out_proj.bias")]
    r = R.classify(hidden.cpu().double().numpy(), frame_lens, mode, *W, labels, k1.cpu().double().numpy() * s1, k2.cpu().double().numpy() * s2)
    assert np.array_equal(out.frame_lens.cpu().numpy(), frame_lens)

    seen = {}
    run = model.encoder.backward_hidden
    model.encoder.backward_hidden = lambda d: (seen.update(dhidden=d.clone()), run(d))[1]
    model.head_grads.fill_(float("nan"))
    model.backward(grad_scale=gs)
    bar = 2.0 ** -12

    def dist(got, want):
        want = np.asarray(want, dtype=np.float64)
        return float(np.abs(got.cpu().double().numpy() - want).max() / np.abs(want).max())
    d = dict(logits=dist(out.logits, r["logits"]), probs=dist(out.probs, r["probs"]), loss=dist(out.loss, [r["loss"]]),
             dW1=dist(model.head_grad("classifier.dense.weight"), gs * r["dW1"]), db1=dist(model.head_grad("classifier.dense.bias"), gs * r["db1"]),
             dW2=dist(model.head_grad("classifier.out_proj.weight"), gs * r["dW2"]), db2=dist(model.head_grad("classifier.out_proj.bias"), gs * r["db2"]))
    print(f"classifier lengths/dropout/grad_scale {mode}:", d)
    assert all(v <= bar for v in d.values()), d
    want = gs * r["dhidden"]
    got = seen["dhidden"].cpu().double().numpy()
    assert seen["dhidden"].dtype == torch.bfloat16 and got.shape == want.shape
    assert (np.abs(got - want) <= HALF_BF16_ULP * np.abs(want) + bar * np.abs(want).max()).all()
    assert (got[1, frame_lens[1]:] == 0).all() and (got[want == 0] == 0).all()
    last = f"wav2vec2.encoder.layers.{model.config.num_hidden_layers - 1}.final_layer_norm.weight"
    g = model.grad(last)
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0  # the encoder's backward ran from that d hidden


def test_command_line_prints_scores_as_json(golden, capsys):
    from ssak_amd.classify import main
    z, folder = golden
    wav = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bonjour.wav")
    main([wav, wav, "--model", folder, "--start", "0.2", "--end", "1.0"])
    text = capsys.readouterr().out
    docs, dec, pos = [], json.JSONDecoder(), 0
    while pos < len(text.rstrip()):
        obj, pos = dec.raw_decode(text, pos)
        docs.append(obj)
        pos += len(text[pos:]) - len(text[pos:].lstrip())
    assert len(docs) == 2 and docs[0] == docs[1]  # one object per file, and the same file scores the same
    assert set(docs[0]) == {"m", "f"} and abs(sum(docs[0].values()) - 1) < 1e-6
    main([wav, "--model", folder])
    whole = json.loads(capsys.readouterr().out)
    assert set(whole) == {"m", "f"} and whole != docs[0]  # the cut changes what is scored
