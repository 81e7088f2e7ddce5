"""GPU: LoRA fine-tuning composed -- WhisperSeq2Seq.add_lora / forward_train / backward (frozen base), WhisperAdamW on the adapters,
merge / unmerge, adapter folders and run_training(lora=...) -- on the tiny golden model (D 128, 2 heads, 2 layers, V 127, B 3, L 12,
S 50, encoder lengths 50 / 50 / 23) with r = 8, lora_alpha = 16, against the float64 restatement tests/whisper_lora_ref.py (itself
held to tests/whisper_train_ref.py and to transformers by tests/test_whisper_lora_ref.py).

Bars are measured, not chosen: ``check_grads`` of tests/test_gpu_whisper_train.py -- per tensor min(4 x d, 6e-2) relative L2, d the
distance between the restatement with the device's storage roundings and in float64.  Every test prints what it measured first.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_whisper_dec as G  # noqa: E402
import whisper_decoder_ref as WR  # noqa: E402
import whisper_lora_ref as LR  # noqa: E402
import whisper_train_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAD_BAR = 6e-2
R_, ALPHA = 8, 16.0
SCALING = ALPHA / R_
ROWS = {0: G.B * G.L, 1: G.B * G.L, 2: G.B * G.L, 3: G.B * G.S}  # rows of each adapter's input, by ``which``


@pytest.fixture(scope="module")
def golden():
    g = np.load(G.GOLDEN)
    return dict(g=g, w={k[2:]: WR.bf16_from_bits(g[k]) for k in g.files if k.startswith("w/")}, enc=WR.bf16_from_bits(g["enc"]),
                labels=WR.shifted_targets(g["tokens"], g["lens"]), enc_lens=[int(v) for v in g["enc_lens"]])


@pytest.fixture(scope="module")
def folder(golden, tmp_path_factory):
    return G.write_folder(golden["g"], str(tmp_path_factory.mktemp("whisper_lora_tiny")))


@pytest.fixture(scope="module")
def lora():
    return LR.random_lora(G.LAYERS, G.D, R_, seed=5)


def restate(golden, lora, **kw):
    a = golden
    return LR.decoder_loss_and_lora_grads(a["w"], lora, G.NH, G.LAYERS, a["enc"], a["labels"], a["enc_lens"], G.EOT, G.SOT, scaling=SCALING, **kw)


@pytest.fixture(scope="module")
def ref(golden, lora):
    return {key: restate(golden, lora, storage=st) for key, st in (("f64", False), ("dev", True))}


def load(folder, lora=None, dropout=0.0, seed=42):
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq
    m = WhisperSeq2Seq.from_pretrained(folder)
    m.add_lora(r=R_, alpha=ALPHA, dropout=dropout, seed=seed)
    if lora is not None:
        m.load_lora_state_dict({k: torch.from_numpy(v.astype(np.float32)) for k, v in lora.items()})
    return m


def dev_enc(golden):
    return torch.from_numpy(golden["enc"].astype(np.float32)).to(torch.bfloat16).to(DEV)


def step(m, golden):
    loss = m.forward_train(dev_enc(golden), golden["labels"], golden["enc_lens"])
    assert m.backward() is None
    torch.cuda.synchronize()
    return loss


def lora_grads_by_name(m):
    torch.cuda.synchronize()
    return {n: m.lora_grad(n).double().cpu().numpy() for n in LR.names(G.LAYERS)}


def check(name, got_loss, got, want, dev):
    d = abs(dev[0] - want[0])
    print(f"{name}: loss {got_loss:.6f}, float64 {want[0]:.6f}: err {abs(got_loss - want[0]):.3e}, measured storage distance {d:.3e}, bar {4 * d:.3e}")
    worst = ("", 0.0)
    for n, w in want[1].items():
        dd = TR.rel_l2(dev[1][n], w)
        bar = min(4 * dd, GRAD_BAR)
        e = TR.rel_l2(got[n], w)
        print(f"{name} {n}: rel L2 {e:.3e}, measured storage distance {dd:.3e}, bar {bar:.3e}, err/bar {e / bar:.3f}")
        if e / bar > worst[1]:
            worst = (n, e / bar)
    print(f"{name}: worst err/bar {worst[1]:.3f} ({worst[0]})")
    assert abs(got_loss - want[0]) <= 4 * d
    for n, w in want[1].items():
        assert TR.rel_l2(got[n], w) <= min(4 * TR.rel_l2(dev[1][n], w), GRAD_BAR), n


def test_loss_and_adapter_gradients_without_dropout(folder, golden, lora, ref):
    m = load(folder, lora)
    assert m.freeze_encoder and m.lora_params.numel() == G.LAYERS * 4 * 2 * R_ * G.D
    loss = step(m, golden)
    assert loss.dtype == torch.float32 and loss.is_cuda
    check("p = 0", float(loss.item()), lora_grads_by_name(m), ref["f64"], ref["dev"])
    assert m._dec_grads is None


def test_loss_and_adapter_gradients_with_dropout(folder, golden, lora):
    """p = 0.5: the device's masks, fetched by site and seed, go into the restatement."""
    from ssak_amd import hip
    p = 0.5
    m = load(folder, lora, dropout=p, seed=7)
    loss = step(m, golden)
    seed = m.lora_drop_seed
    masks = {(l, k): hip.debug_dropout_mask(seed, m.lora_site(l, k), p, ROWS[k], G.D, DEV)[0].cpu().numpy() for l in range(G.LAYERS) for k in range(4)}
    frac = np.mean([v.mean() for v in masks.values()])
    print(f"kept fraction over the {len(masks)} sites: {frac:.4f}")
    assert 0.45 < frac < 0.55
    res = {key: restate(golden, lora, storage=st, masks=masks, mask_scale=LR.drop_scale(p)) for key, st in (("f64", False), ("dev", True))}
    check("p = 0.5", float(loss.item()), lora_grads_by_name(m), res["f64"], res["dev"])
    # validation: no dropout, nothing kept, the step counter stays
    before = m.lora_step
    val = m.forward_train(dev_enc(golden), golden["labels"], golden["enc_lens"], keep_graph=False)
    m0 = load(folder, lora)
    val0 = m0.forward_train(dev_enc(golden), golden["labels"], golden["enc_lens"], keep_graph=False)
    assert torch.equal(val, val0) and m.lora_step == before and m._train is None


def test_zero_B_is_the_base_model(folder, golden):
    """PEFT's initial state: B = 0.  The loss is the base model's bit for bit and no gradient reaches A."""
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq
    base = WhisperSeq2Seq.from_pretrained(folder)
    want = base.forward_train(dev_enc(golden), golden["labels"], golden["enc_lens"], keep_graph=False)
    m = load(folder, None, dropout=0.05)
    A = m.lora_param(LR.names(G.LAYERS)[0]).double().cpu().numpy()
    assert np.abs(A).max() <= 1 / np.sqrt(G.D) and np.abs(A).max() > 0.9 / np.sqrt(G.D) and abs(A.mean()) < 0.1 / np.sqrt(G.D), "A ~ U(+-1/sqrt(D_in))"
    loss = step(m, golden)
    assert torch.equal(loss, want), (float(loss), float(want))
    for n, g in lora_grads_by_name(m).items():
        if ".lora_A." in n:
            assert (g == 0).all(), n
        else:
            assert np.abs(g).max() > 0, n


def test_the_base_stays_frozen(folder, golden, lora):
    from ssak_amd.whisper_train import WhisperAdamW
    m = load(folder, lora, dropout=0.05)
    frozen = [m.dec_params, m.dec_shadow, m.encoder.params, m.encoder.shadow]
    before = [t.clone() for t in frozen]
    lora_before = m.lora_params.clone()
    opt = WhisperAdamW(m, lr=1e-3, warmup_steps=0)
    assert len(opt.halves) == 1 and opt.exp_avg[0].numel() == m.lora_params.numel(), "moments for the adapters only"
    feats = torch.from_numpy(np.random.default_rng(4).standard_normal((G.B, G.MELS, 2 * G.S)).astype(np.float32))
    m.forward_train(feats, golden["labels"])  # through the (frozen) encoder
    assert m.backward() is None
    opt.step()
    torch.cuda.synchronize()
    for t, b in zip(frozen, before):
        assert torch.equal(t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32), b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))
    assert m._dec_grads is None and not m.encoder_grads_ready
    assert not torch.equal(lora_before, m.lora_params), "the adapters did not move"
    assert torch.equal(m.lora_params.to(torch.bfloat16).view(torch.int16), m.lora_shadow.view(torch.int16)), "the bf16 shadow follows the step"
    norm = float(m.lora_grads.double().norm())
    print(f"clip norm {opt.grad_norm():.6f}, adapter gradient norm {norm:.6f}")
    assert abs(opt.grad_norm() - norm) <= 1e-5 * norm, "the clip norm runs over the adapter gradients alone"


def test_a_step_is_repeatable_and_consecutive_steps_draw_new_masks(folder, golden, lora):
    from ssak_amd import hip
    m = load(folder, lora, dropout=0.5, seed=11)
    out = []
    for _ in range(2):
        m.lora_step = 0
        loss = step(m, golden)
        out.append((loss.clone(), m.lora_grads.clone(), m.lora_drop_seed))
    assert out[0][2] == out[1][2] and torch.equal(out[0][0], out[1][0]), "two runs differ"
    assert torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32)), "two runs differ"
    step(m, golden)
    assert m.lora_step == 2 and m.lora_drop_seed != out[0][2]
    k1 = hip.debug_dropout_mask(out[0][2], m.lora_site(0, 0), 0.5, ROWS[0], G.D, DEV)[0]
    k2 = hip.debug_dropout_mask(m.lora_drop_seed, m.lora_site(0, 0), 0.5, ROWS[0], G.D, DEV)[0]
    assert not torch.equal(k1, k2)
    assert not torch.equal(out[0][1], m.lora_grads), "the second step's gradients are the first's"
    assert len({m.lora_site(l, k) for l in range(32) for k in range(4)}) == 128 and min(m.lora_site(l, k) for l in range(32) for k in range(4)) >= 16 + 4 * 32 + 4


def test_ten_step_curve_follows_the_reference(folder, golden, lora):
    """One fixed batch, AdamW on the adapters (lr 1e-3, no warm-up, weight decay 0.01 on every adapter weight, clip 1.0), 10 steps,
    p = 0.  Reference: the float64 restatement under torch.optim.AdamW.  Bar: 4 x the largest distance between that curve and the
    same reference with A / B re-rounded to bf16 for each forward (the engine's shadow) -- the existing 20-step test's rule."""
    from ssak_amd.trainer import linear_warmup_lr
    from ssak_amd.whisper_train import WhisperAdamW
    steps, lr, total = 10, 1e-3, 1000
    curves = {}
    for key, rl in (("f64", False), ("shadow", True)):
        params = {k: torch.tensor(v, requires_grad=True) for k, v in lora.items()}
        opt = torch.optim.AdamW(list(params.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
        curve = []
        for i in range(steps):
            for gr in opt.param_groups:
                gr["lr"] = linear_warmup_lr(lr, i, 0, total)
            opt.zero_grad()
            loss = restate(golden, None, params=params, round_lora=rl)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
            opt.step()
            curve.append(float(loss.detach()))
        curves[key] = np.array(curve)
    m = load(folder, lora)
    opt = WhisperAdamW(m, lr=lr, weight_decay=0.01, warmup_steps=0, total_steps=total, max_grad_norm=1.0)
    enc = dev_enc(golden)
    losses = []
    for i in range(steps):
        losses.append(m.forward_train(enc, golden["labels"], golden["enc_lens"]))
        m.backward()
        opt.step()
    dev = torch.cat(losses).double().cpu().numpy()
    d = float(np.abs(curves["shadow"] - curves["f64"]).max())
    e = float(np.abs(dev - curves["f64"]).max())
    print("step  device      float64     float64 + bf16 shadow")
    for i in range(steps):
        print(f"{i:4d}  {dev[i]:.6f}  {curves['f64'][i]:.6f}  {curves['shadow'][i]:.6f}")
    print(f"10-step curve: max |device - float64| {e:.3e}, measured distance to the shadowed reference {d:.3e}, bar {4 * d:.3e}, err/bar {e / (4 * d):.3f}")
    assert dev[-1] < dev[0] and curves["f64"][-1] < curves["f64"][0]
    assert e <= 4 * d


def test_merged_and_unmerged_paths_agree_and_round_trip_through_an_adapter_folder(folder, golden, lora, tmp_path):
    """The two paths compute the same function and round in different places: unmerged stores the base product, t and the sum
    (three bf16 roundings around the adapter), merged rounds W + s B A once.  Each path's distance to the float64 function is
    measured on the CPU with exactly its roundings (d_u, d_m: relative L2 of the logits); by the triangle inequality the two device
    paths are within 4 d_u + 4 d_m of each other under the 4 x rule every other bar here uses."""
    a = golden
    m = load(folder, lora)
    ids = TR.shift_tokens_right(a["labels"], G.EOT, G.SOT)
    enc = dev_enc(golden)
    unmerged = m.decode_logits(enc, ids, a["enc_lens"]).double().cpu().numpy()
    with m.lora_merged():
        merged = m.decode_logits(enc, ids, a["enc_lens"]).double().cpu().numpy()
        gen_merged = m.generate(enc, language="en", max_new_tokens=8, enc_lens=a["enc_lens"])
    gen_auto = m.generate(enc, language="en", max_new_tokens=8, enc_lens=a["enc_lens"])  # (merges for the call)
    assert not m._lora_merged and gen_auto.tokens == gen_merged.tokens
    f64 = restate(golden, lora, want_logits=True)
    l_u = restate(golden, lora, want_logits=True, storage=True)
    w_m = dict(a["w"])
    for n in lora:
        if n.endswith(".lora_A.weight"):
            mod = n[:-len(".lora_A.weight")]
            w_m[mod + ".weight"] = TR._bf16(torch.from_numpy(a["w"][mod + ".weight"] + SCALING * (lora[mod + ".lora_B.weight"] @ lora[n]))).numpy()
    l_m = LR.decoder_loss_and_lora_grads(w_m, {k: np.zeros_like(v) for k, v in lora.items()}, G.NH, G.LAYERS, a["enc"], a["labels"], a["enc_lens"],
                                         G.EOT, G.SOT, scaling=SCALING, storage=True, want_logits=True)
    base = LR.decoder_loss_and_lora_grads(a["w"], {k: np.zeros_like(v) for k, v in lora.items()}, G.NH, G.LAYERS, a["enc"], a["labels"], a["enc_lens"],
                                          G.EOT, G.SOT, scaling=SCALING, want_logits=True)
    d_u, d_m = TR.rel_l2(l_u, f64), TR.rel_l2(l_m, f64)
    e = TR.rel_l2(merged, unmerged)
    print(f"logits: merged vs unmerged rel L2 {e:.3e}; measured d_u {d_u:.3e}, d_m {d_m:.3e}, bar {4 * (d_u + d_m):.3e}, err/bar {e / (4 * (d_u + d_m)):.3f}; "
          f"the adapters move the logits by {TR.rel_l2(f64, base):.3e}; unmerged vs float64 {TR.rel_l2(unmerged, f64):.3e}, merged {TR.rel_l2(merged, f64):.3e}")
    # what the comparison can see: a path that dropped its adapters would sit at the adapters' own effect on the logits (float64,
    # with against without), so that effect has to lie above the bar
    assert TR.rel_l2(f64, base) > 4 * (d_u + d_m), "the adapters are too small for this test to see them"
    assert e <= 4 * (d_u + d_m)
    assert TR.rel_l2(unmerged, f64) <= 4 * d_u and TR.rel_l2(merged, f64) <= 4 * d_m
    # the adapter folder: base_model_name_or_path = the tiny folder; from_pretrained merges it with the same kernel
    out = m.save_adapter(str(tmp_path / "ckpt" / "adapter_model"))
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq
    m2 = WhisperSeq2Seq.from_pretrained(str(tmp_path / "ckpt"))  # (found below the folder, as the reference walks it)
    assert m2._lora is None and os.path.samefile(out, str(tmp_path / "ckpt" / "adapter_model"))
    with m.lora_merged():
        torch.cuda.synchronize()
        assert torch.equal(m.dec_shadow.view(torch.int16), m2.dec_shadow.view(torch.int16)), "the loaded shadow is the merged shadow"
    gen_loaded = m2.generate(enc, language="en", max_new_tokens=8, enc_lens=a["enc_lens"])
    print("tokens:", gen_merged.tokens)
    assert gen_loaded.tokens == gen_merged.tokens
    base_gen = WhisperSeq2Seq.from_pretrained(folder).generate(enc, language="en", max_new_tokens=8, enc_lens=a["enc_lens"])
    print("base tokens:", base_gen.tokens)
    with pytest.raises(ValueError, match="not built"):
        WhisperSeq2Seq.from_pretrained(folder).add_lora(r=R_, target_modules=["k_proj"])
    with pytest.raises(RuntimeError, match="merged"):
        with m.lora_merged():
            m.forward_train(enc, a["labels"], a["enc_lens"])


def test_training_loop_with_lora_on_a_synthetic_kaldi_folder(golden, tmp_path):
    """run_training(lora=...) on three 1 s synthetic utterances with a stub tokenizer: two steps, a validation (loss unmerged, WER on
    the merged shadow) with an adapter checkpoint, the final adapter folder, which loads."""
    from safetensors.torch import load_file
    from ssak_amd.data import load_kaldi
    from ssak_amd.synth import write_kaldi_folder
    from ssak_amd.train_whisper import run_training
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq
    data = str(tmp_path / "kaldi")
    write_kaldi_folder(data, 3, seconds=1.0, seed=11, threads=2)
    utts = load_kaldi(data)
    assert len(utts) == 3
    base = G.write_folder(golden["g"], str(tmp_path / "model"), max_source_positions=1500, encoder_layers=1)
    m = WhisperSeq2Seq.from_pretrained(base)
    tokenize = lambda text: [G.SOT] + [ord(c) % 90 for c in text[:9]] + [G.EOT]
    out = str(tmp_path / "out")
    recs = run_training(m, utts, utts[:2], tokenize, batch_size=2, learning_rate=1e-3, warmup_steps=0, num_epochs=1, max_steps=2, eval_steps=2,
                        output_dir=out, detokenize=lambda ids: " ".join(chr(97 + i % 26) for i in ids), log=lambda rec: print(rec),
                        lora=dict(r=R_, alpha=ALPHA, dropout=0.05))
    steps = [r for r in recs if "loss" in r]
    evals = [r for r in recs if "eval_loss" in r]
    assert [r["step"] for r in steps] == [1, 2] and all(np.isfinite(r["loss"]) and r["grad_norm"] > 0 for r in steps)
    assert [r["step"] for r in evals] == [0, 2] and all(np.isfinite(r["eval_loss"]) and np.isfinite(r["eval_wer"]) for r in evals)
    assert m._lora is not None and m._dec_grads is None and not m._lora_merged
    ckpt = os.path.join(out, "checkpoint-2", "adapter_model")
    assert os.path.isfile(os.path.join(ckpt, "adapter_model.safetensors")) and os.path.isfile(os.path.join(ckpt, "adapter_config.json"))
    assert not os.path.exists(os.path.join(out, "model.safetensors")), "only the adapter is saved"
    assert os.path.isfile(os.path.join(out, "adapter_model.safetensors")) and os.path.isfile(os.path.join(out, "generation_config.json"))
    sd = load_file(os.path.join(out, "adapter_model.safetensors"))
    torch.cuda.synchronize()
    for n in LR.names(G.LAYERS):
        assert torch.equal(sd["base_model.model." + n], m.lora_param(n).cpu()), n
    assert any(bool((sd["base_model.model." + n] != 0).any()) for n in LR.names(G.LAYERS) if ".lora_B." in n), "B moved off zero"
    m2 = WhisperSeq2Seq.from_pretrained(out)
    with m.lora_merged():
        torch.cuda.synchronize()
        assert torch.equal(m.dec_shadow.view(torch.int16), m2.dec_shadow.view(torch.int16))
