"""Fine-tuning of a Whisper model on Kaldi folders, on one MI355X (the reference's ssak/train/transformers/whisper_train.py): every
parameter (its non-PEFT branch) or, with ``--lora``, the reference's LoRA adapters on the bf16 base::

    python -m ssak_amd.train_whisper TRAIN VALID --base_model DIR [--lang fr] [--task transcribe] [--batch_size 8] [--batch_size_eval N]
                                     [--learning_rate 1e-5] [--weight_decay 0.01] [--warmup_steps N] [--num_epochs 3] [--max_steps N]
                                     [--seed 42] [--max_duration 30] [--min_duration 0.1] [--max_text_length 448] [--eval_steps N]
                                     [--disable_first_eval] [-o OUTPUT_DIR] [--overwrite_output_dir] [--freeze_encoder]
                                     [--lora [--lora_r 32] [--lora_alpha 64] [--lora_dropout 0.05]]

``TRAIN`` / ``VALID``: a Kaldi folder, several separated by commas, or a list file (:mod:`ssak_amd.data`).  ``DIR`` is a
``WhisperForConditionalGeneration`` folder in the HuggingFace layout WITH its tokenizer files (nothing is downloaded): labels are
``transformers.WhisperTokenizer(text)`` with the language and task prefix, as the reference's collator makes them.  Audio goes
through the device log-mel (:meth:`WhisperSeq2Seq.features`), the step is :meth:`WhisperSeq2Seq.forward_train` / ``backward`` and
:class:`ssak_amd.whisper_train.WhisperAdamW` (one global-norm clip at 1.0, HF's two weight-decay groups, linear warm-up -- 1 % of
the steps by default -- and decay).  Every ``--eval_steps`` steps (default: every epoch), and before the first step unless
``--disable_first_eval``, validation reports ``eval_loss`` (teacher-forced) and the WER of :meth:`WhisperSeq2Seq.generate`
(:func:`ssak_amd.metrics.text_wer`), and a checkpoint is written (``save_pretrained``: a folder ``from_pretrained`` and transformers
read).  ``--lora``: adapters on the decoder's ``q_proj`` / ``v_proj`` (:meth:`WhisperSeq2Seq.add_lora`), the base frozen; the checkpoints
are PEFT adapter folders (``checkpoint-<step>/adapter_model/``, and ``adapter_config.json`` + ``adapter_model.safetensors`` with the
tokenizer files in the output folder), which ``from_pretrained`` -- and so ``python -m ssak_amd.whisper_infer`` -- loads merged.

Differences from the reference, each refused by name where it is asked for: ``--gradient_accumulation_steps`` defaults to 1 here
(16 there) and no other value is built; ``--peft`` (int8 + LoRA), ``--int4``, ``--data_augmentation`` and ``--text_augmentation`` are not
built.
One GPU; no data parallelism.

:func:`run_training` is the loop itself: it takes utterances, a ``tokenize`` callable (text -> label ids) and, for the WER, a
``detokenize`` callable (ids -> text), so it runs without a tokenizer.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import math
import os
import shutil
import sys
import time
from typing import Callable, List, Optional, Sequence

import numpy as np

_NOT_BUILT = {"peft": "--peft: the reference's int8 + LoRA branch is not built; `--lora` trains the same adapters on the bf16 base",
              "int4": "--int4: 4-bit quantisation is not built",
              "data_augmentation": "--data_augmentation: audio augmentation is not wired into Whisper fine-tuning (python -m ssak_amd.train "
                                   "--data_augment has it for wav2vec2)",
              "text_augmentation": "--text_augmentation: text augmentation is not built"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ssak_amd.train_whisper", description="Fine-tune a Whisper model (all parameters) on Kaldi folders.")
    ap.add_argument("train", help="a Kaldi folder, or a file listing Kaldi folders, with the training data")
    ap.add_argument("valid", help="a Kaldi folder, or a file listing Kaldi folders, with the validation data")
    ap.add_argument("--base_model", required=True, metavar="DIR", help="Whisper model folder to tune (HuggingFace layout, with its tokenizer)")
    ap.add_argument("--lang", default="fr", help="language to tune")
    ap.add_argument("--task", default="transcribe", choices=("transcribe", "translate"))
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--batch_size_eval", type=int, default=None, help="batch size of the validation (default: --batch_size)")
    ap.add_argument("--learning_rate", type=float, default=1e-5)
    ap.add_argument("--gradient_accumulation_steps", type=int, default=1, help="only 1 is built (the reference's default is 16)")
    ap.add_argument("--num_epochs", type=int, default=3)
    ap.add_argument("--max_steps", type=int, default=None, help="stop after this many optimizer steps")
    ap.add_argument("--weight_decay", type=float, default=0.01)
    ap.add_argument("--warmup_steps", type=int, default=None, help="default: 1 %% of the steps")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--max_duration", type=float, default=30, help="longest training utterance, seconds")
    ap.add_argument("--min_duration", type=float, default=0.1, help="shortest training utterance, seconds")
    ap.add_argument("--max_text_length", type=int, default=448, help="most label tokens per utterance")
    ap.add_argument("--eval_steps", type=int, default=None, help="validate and checkpoint every N steps (default: every epoch)")
    ap.add_argument("--disable_first_eval", action="store_true", help="do not validate the initial model")
    ap.add_argument("-o", "--output_dir", default=".", help="parent folder of the output folder")
    ap.add_argument("--overwrite_output_dir", action="store_true")
    ap.add_argument("--freeze_encoder", action="store_true", help="train the decoder only")
    ap.add_argument("--lora", action="store_true", help="train LoRA adapters on the decoder's q_proj / v_proj (bf16 base, everything else frozen)")
    ap.add_argument("--lora_r", type=int, default=32)
    ap.add_argument("--lora_alpha", type=float, default=64)
    ap.add_argument("--lora_dropout", type=float, default=0.05)
    ap.add_argument("--device", default="cuda:0")
    for flag in _NOT_BUILT:
        ap.add_argument("--" + flag, action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    for flag, why in _NOT_BUILT.items():
        if getattr(args, flag):
            ap.error(why)
    if args.gradient_accumulation_steps != 1:
        ap.error(f"--gradient_accumulation_steps {args.gradient_accumulation_steps}: gradient accumulation is not built; the step is one batch "
                 f"(the default here is 1, the reference's is 16: raise --batch_size instead)")
    if args.batch_size < 1 or (args.batch_size_eval is not None and args.batch_size_eval < 1):
        ap.error("--batch_size and --batch_size_eval must be at least 1")
    if args.lora_r not in (8, 16, 32, 64) or not 0.0 <= args.lora_dropout < 1.0:
        ap.error("--lora_r must be 8, 16, 32 or 64 and --lora_dropout in [0, 1)")
    if args.max_text_length < 1 or args.num_epochs < 1:
        ap.error("--max_text_length and --num_epochs must be at least 1")
    args.batch_size_eval = args.batch_size_eval or args.batch_size
    return args


def make_labels(texts: Sequence[str], tokenize: Callable[[str], List[int]], decoder_start_token_id: int):
    """Label ids per utterance as the reference's collator makes them: the tokenizer's ids, without the leading
    ``<|startoftranscript|>`` when every sequence starts with it (``shift_tokens_right`` puts it back)."""
    ids = [list(tokenize(t)) for t in texts]
    if ids and all(i and i[0] == decoder_start_token_id for i in ids):
        ids = [i[1:] for i in ids]
    return ids


def _batch(utts, labels):
    from .data import load_audio, pad_labels, pad_waves
    import torch
    waves, _ = pad_waves([load_audio(u.path, u.start, u.end) for u in utts])
    return torch.from_numpy(waves), pad_labels(labels, -100)


def evaluate(model, utts, labels, batch_size: int, detokenize=None, language=None, task="transcribe") -> dict:
    """``eval_loss``: the teacher-forced cross-entropy over every scored token of the set; with ``detokenize`` also ``eval_wer`` of
    greedy :meth:`WhisperSeq2Seq.generate` against the utterances' texts."""
    from .metrics import text_wer
    total, n_tok, refs, hyps = 0.0, 0, [], []
    for i in range(0, len(utts), batch_size):
        u, lab = utts[i:i + batch_size], labels[i:i + batch_size]
        waves, padded = _batch(u, lab)
        n = int((padded >= 0).sum())
        enc = model.encode(model.features(waves))
        total += float(model.forward_train(enc, padded, keep_graph=False).item()) * n
        n_tok += n
        if detokenize is not None:
            with model.lora_merged() if model._lora is not None else contextlib.nullcontext():
                res = model.generate(enc, language=language, task=task)
            refs += [x.text for x in u]
            hyps += [detokenize(t) for t in res.tokens]
    out = {"eval_loss": total / max(n_tok, 1), "eval_tokens": n_tok}
    if detokenize is not None:
        out["eval_wer"] = text_wer(refs, hyps)["wer"]
    return out


def run_training(model, train_utts, valid_utts, tokenize, *, batch_size=8, batch_size_eval=None, learning_rate=1e-5, weight_decay=0.01,
                 warmup_steps=None, num_epochs=3, max_steps=None, seed=42, max_text_length=448, eval_steps=None, disable_first_eval=False,
                 output_dir=None, detokenize=None, language=None, task="transcribe", log=None, lora: Optional[dict] = None) -> List[dict]:
    """The training loop -> the log records (dicts; ``log`` is called with each).  Utterances whose labels exceed
    ``max_text_length`` tokens are dropped, as the reference's filter does.  With ``output_dir`` a checkpoint
    ``checkpoint-<step>`` is written at every validation and the final model into ``output_dir`` itself.  ``lora`` (the arguments
    of :meth:`WhisperSeq2Seq.add_lora`; {} for the reference's): the adapters are trained on the frozen base and the checkpoints are
    adapter folders, ``checkpoint-<step>/adapter_model/`` and, in ``output_dir``, the adapter next to the tokenizer files."""
    from .whisper_train import _TOKENIZER_FILES, TRAIN_ROW_CHUNK, WhisperAdamW
    if lora is not None and model._lora is None:
        model.add_lora(**dict({"seed": seed}, **lora))
    model.row_chunk = max(model.row_chunk, TRAIN_ROW_CHUNK)
    log = log or (lambda rec: print(json.dumps(rec), flush=True))
    start = model.config.decoder_start_token_id
    cap = min(max_text_length, model.config.max_target_positions)

    def prepare(utts):
        labs = make_labels([u.text for u in utts], tokenize, start)
        keep = [i for i, l in enumerate(labs) if 1 <= len(l) <= cap]
        return [utts[i] for i in keep], [labs[i] for i in keep]

    train_utts, train_labels = prepare(train_utts)
    valid_utts, valid_labels = prepare(valid_utts)
    if not train_utts:
        raise ValueError("no training utterance is left after the duration and text-length filters")
    per_epoch = math.ceil(len(train_utts) / batch_size)
    total = per_epoch * num_epochs if max_steps is None else min(max_steps, per_epoch * num_epochs)
    warmup = max(1, total // 100) if warmup_steps is None else warmup_steps
    eval_every = per_epoch if eval_steps is None else eval_steps
    opt = WhisperAdamW(model, lr=learning_rate, weight_decay=weight_decay, max_grad_norm=1.0, warmup_steps=warmup, total_steps=total)
    records = []

    def emit(rec):
        records.append(rec)
        log(rec)

    def validate(step):
        rec = {"step": step}
        if valid_utts:
            rec.update(evaluate(model, valid_utts, valid_labels, batch_size_eval or batch_size, detokenize, language, task))
        if output_dir is not None:
            ckpt = os.path.join(output_dir, f"checkpoint-{step}")
            rec["checkpoint"] = model.save_pretrained(ckpt) if lora is None else model.save_adapter(os.path.join(ckpt, "adapter_model"))
        emit(rec)

    if not disable_first_eval and valid_utts:
        emit(dict({"step": 0}, **evaluate(model, valid_utts, valid_labels, batch_size_eval or batch_size, detokenize, language, task)))
    rng = np.random.RandomState(seed)
    step, t0 = 0, time.time()
    for epoch in range(num_epochs):
        order = rng.permutation(len(train_utts))
        for i in range(0, len(order), batch_size):
            idx = order[i:i + batch_size]
            waves, padded = _batch([train_utts[j] for j in idx], [train_labels[j] for j in idx])
            lr = opt.current_lr()
            loss = model.forward_train(waves, padded)
            model.backward()
            opt.step()
            step += 1
            emit({"step": step, "epoch": epoch + i / max(len(order), 1), "loss": float(loss.item()), "learning_rate": lr,
                  "grad_norm": opt.grad_norm(), "elapsed_s": time.time() - t0})
            if step % eval_every == 0 or step == total:
                validate(step)
            if step == total:
                break
        if step == total:
            break
    if output_dir is not None and lora is None:
        model.save_pretrained(output_dir)
    elif output_dir is not None:
        model.save_adapter(output_dir)
        src = model.name_or_path
        for name in _TOKENIZER_FILES if src is not None and os.path.abspath(src) != os.path.abspath(output_dir) else ():
            if os.path.isfile(os.path.join(src, name)):
                shutil.copyfile(os.path.join(src, name), os.path.join(output_dir, name))
    return records


def main(argv=None):
    args = parse_args(argv)
    from .data import load_kaldi
    from .whisper_infer import _tokenizer
    from .whisper_seq2seq import WhisperSeq2Seq
    tok = _tokenizer(args.base_model)
    if tok is None:
        raise SystemExit(f"train_whisper: {args.base_model} holds no tokenizer that transformers.WhisperTokenizer can read (vocab.json, merges.txt, "
                         f"...), or transformers is not installed: the labels are the tokenizer's ids.  ssak_amd.train_whisper.run_training() "
                         f"takes label ids from any tokenize callable.")
    tok.set_prefix_tokens(language=args.lang, task=args.task)
    name = f"{os.path.basename(os.path.normpath(args.base_model))}_{args.lang}_lr{args.learning_rate}_bs{args.batch_size}"
    out = os.path.join(args.output_dir, name)
    if os.path.isdir(out) and os.listdir(out) and not args.overwrite_output_dir:
        raise SystemExit(f"train_whisper: {out} exists and is not empty: pass --overwrite_output_dir")
    os.makedirs(out, exist_ok=True)
    model = WhisperSeq2Seq.from_pretrained(args.base_model, device=args.device, freeze_encoder=args.freeze_encoder)
    train = load_kaldi(args.train, min_duration=args.min_duration, max_duration=args.max_duration)
    valid = load_kaldi(args.valid)
    print(f"train_whisper: {len(train)} training and {len(valid)} validation utterances; output {out}", file=sys.stderr)
    run_training(model, train, valid, lambda text: tok(text).input_ids, batch_size=args.batch_size, batch_size_eval=args.batch_size_eval,
                 learning_rate=args.learning_rate, weight_decay=args.weight_decay, warmup_steps=args.warmup_steps, num_epochs=args.num_epochs,
                 max_steps=args.max_steps, seed=args.seed, max_text_length=args.max_text_length, eval_steps=args.eval_steps,
                 disable_first_eval=args.disable_first_eval, output_dir=out, detokenize=lambda ids: tok.decode(ids, skip_special_tokens=True).strip(),
                 language=args.lang, task=args.task,
                 lora=dict(r=args.lora_r, alpha=args.lora_alpha, dropout=args.lora_dropout) if args.lora else None)


if __name__ == "__main__":
    main()
