"""Transcription with a Whisper model on the GPU, greedy, by beam search or by sampling with whisper's temperature fallback (what
ssak/infer/whisper_infer.py asks of ``model.transcribe``, ``condition_on_previous_text = False``)::

    python -m ssak_amd.whisper_infer AUDIO... --model DIR [--language fr] [--task transcribe] [--max_new_tokens N] [--batch_size N]
                                     [--timestamps] [--beam_size N] [--temperature T] [--temperature_increment_on_fallback I]
                                     [--best_of N] [--compression_ratio_threshold R] [--logprob_threshold L] [--no_speech_threshold P]
                                     [--seed S] [--accurate]

prints one line per file, ``path<TAB>ids`` (the generated token ids, space-separated, without the prompt) and, where
``transformers.WhisperTokenizer`` can be imported and ``DIR`` holds a tokenizer, ``<TAB>text``.  ``DIR`` is a
``WhisperForConditionalGeneration`` folder in the HuggingFace layout (nothing is downloaded).  Without ``--language`` the language
of each file is detected first.  Audio goes through the device ingest, Whisper's 30 s window and ``ssak_logmel_whisper``, then
:meth:`ssak_amd.whisper_seq2seq.WhisperSeq2Seq.generate`.  Audio longer than 30 s is refused by name unless ``--timestamps`` is given.

``--timestamps`` runs :meth:`ssak_amd.whisper_seq2seq.WhisperSeq2Seq.transcribe` instead -- the timestamp rules, the 30 s window
seeking through a file of any length, silent windows skipped -- and prints one line per segment,
``path<TAB>start<TAB>end<TAB>ids[<TAB>text]`` (seconds; the ids without the timestamp tokens).

``--beam_size N`` (1 to 8) decodes by beam search, with and without ``--timestamps``.  ``--temperature T`` above 0 samples instead,
``--best_of N`` (1 to 8) candidates per file.  ``--temperature_increment_on_fallback I`` makes the schedule
``np.arange(T, 1.0 + 1e-6, I)`` of whisper's fallback: a window whose text compresses beyond ``--compression_ratio_threshold`` or whose
average log-probability is below ``--logprob_threshold`` is decoded again at the next temperature (temperature 0 with the beam, above
0 with ``best_of``); it lives in ``transcribe`` and needs ``--timestamps``.  ``--accurate`` is the reference's shortcut: ``beam_size 5,
best_of 5, increment 0.2``.  The compression ratio is taken of the tokenizer's text; without a tokenizer that check is switched off
with one line on stderr.  ``--seed`` fixes the draws: the same command prints the same lines.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Optional, Tuple

import numpy as np


def _tokenizer(folder: str):
    """``transformers.WhisperTokenizer`` of the model folder, or None where either is missing (the ids are the contract)."""
    if not os.path.isfile(os.path.join(folder, "vocab.json")):
        return None
    try:
        from transformers import WhisperTokenizer
    except ImportError:
        return None
    return WhisperTokenizer.from_pretrained(folder)


def temperature_schedule(temperature: float, increment: Optional[float]) -> Tuple[float, ...]:
    """The reference's schedule: ``np.arange(temperature, 1.0 + 1e-6, increment)`` with an increment, else the one temperature."""
    if increment:
        return tuple(float(t) for t in np.arange(temperature, 1.0 + 1e-6, increment))
    return (float(temperature),)


class _SetAccurate(argparse.Action):
    """``--accurate``: whisper's own defaults, set where the flag stands so that a later flag still overrides them."""

    def __init__(self, option_strings, dest, **kw):
        super().__init__(option_strings, dest, nargs=0, **kw)

    def __call__(self, parser, namespace, values, option_string=None):
        namespace.best_of, namespace.beam_size, namespace.temperature_increment_on_fallback = 5, 5, 0.2


def parse_args(argv=None):
    """The command line -> the namespace, with ``temperatures`` (the schedule as a tuple) on top; refusals by ``ap.error``."""
    ap = argparse.ArgumentParser(prog="python -m ssak_amd.whisper_infer", description="Transcribe each audio file (greedy decoding, up to 30 s).")
    ap.add_argument("audio", nargs="+", metavar="AUDIO", help="PCM WAV file(s), at most 30 s each")
    ap.add_argument("--model", required=True, metavar="DIR", help="Whisper model folder (HuggingFace layout)")
    ap.add_argument("--language", default=None, help="language code (fr, en, ...); by default detected per file")
    ap.add_argument("--task", default="transcribe", choices=("transcribe", "translate"))
    ap.add_argument("--max_new_tokens", type=int, default=None, metavar="N", help="at most N tokens per file (default: what the decoder's positions hold)")
    ap.add_argument("--batch_size", type=int, default=8, metavar="N", help="files per batch")
    ap.add_argument("--device", default="cuda:0", help="GPU to run on")
    ap.add_argument("--timestamps", action="store_true", help="long-form transcription with timestamps: any length, one line per segment")
    ap.add_argument("--beam_size", type=int, default=None, metavar="N", help="beam search with N hypotheses per file (1 to 8; default: greedy)")
    ap.add_argument("--temperature", type=float, default=0.0, metavar="T", help="temperature to sample at (default 0: greedy / beam search)")
    ap.add_argument("--temperature_increment_on_fallback", type=float, default=0.0, metavar="I",
                    help="with --timestamps: decode a failing window again at T + I, T + 2 I, ... up to 1.0 (default 0: no fallback)")
    ap.add_argument("--best_of", type=int, default=None, metavar="N", help="candidates per file when sampling (1 to 8; default 1)")
    ap.add_argument("--compression_ratio_threshold", type=float, default=2.4, metavar="R", help="a window whose text compresses beyond R is decoded again")
    ap.add_argument("--logprob_threshold", type=float, default=-1.0, metavar="L", help="a window whose average log-probability is below L is decoded again")
    ap.add_argument("--no_speech_threshold", type=float, default=0.6, metavar="P", help="a window with no_speech_prob above P (and a low log-probability) is skipped")
    ap.add_argument("--seed", type=int, default=1234, metavar="S", help="seed of the sampling draws")
    ap.add_argument("--accurate", action=_SetAccurate, help="beam_size 5, best_of 5, temperature_increment_on_fallback 0.2")
    args = ap.parse_args(argv)
    if args.beam_size is not None and not 1 <= args.beam_size <= 8:
        ap.error("--beam_size must lie in [1, 8]")
    if args.best_of is not None and not 1 <= args.best_of <= 8:
        ap.error("--best_of must lie in [1, 8]")
    if not args.temperature >= 0.0 or not (args.temperature_increment_on_fallback or 0.0) >= 0.0:
        ap.error("--temperature and --temperature_increment_on_fallback must be >= 0")
    args.temperatures = temperature_schedule(args.temperature, args.temperature_increment_on_fallback)
    if not args.temperatures:
        ap.error(f"--temperature {args.temperature} lies beyond 1.0, where the fallback schedule ends")
    if len(args.temperatures) > 1 and not args.timestamps:
        ap.error("the temperature fallback (--temperature_increment_on_fallback, --accurate) lives in the long-form path: pass --timestamps")
    if args.batch_size < 1:
        ap.error("--batch_size must be at least 1")
    if args.timestamps and args.max_new_tokens is not None:
        ap.error("--max_new_tokens does not apply with --timestamps (a window decodes up to half the decoder's positions)")
    return args


def main(argv=None):
    args = parse_args(argv)
    from .ingest import DeviceIngest
    from .whisper_seq2seq import N_SAMPLES, WhisperSeq2Seq
    model = WhisperSeq2Seq.from_pretrained(args.model, device=args.device)
    tok = _tokenizer(args.model)
    text_of = None if tok is None else (lambda ids: tok.decode(ids, skip_special_tokens=True))
    if tok is None and len(args.temperatures) > 1 and args.compression_ratio_threshold is not None:
        print("whisper_infer: no tokenizer in the model folder: the compression-ratio check of the fallback is off", file=sys.stderr)
    ingest = DeviceIngest(sample_rate=16000, device=args.device, normalize=False)
    for i in range(0, len(args.audio), args.batch_size):
        paths = args.audio[i:i + args.batch_size]
        waves, lens = ingest.load_batch([(p, None, None) for p in paths])
        if args.timestamps:
            ns = lens.cpu().tolist() if hasattr(lens, "cpu") else list(lens)
            ts_begin = model.config.no_timestamps_token_id + 1
            for path, res in zip(paths, model.transcribe([waves[b, :n] for b, n in enumerate(ns)], language=args.language, task=args.task,
                                                         batch_size=args.batch_size, beam_size=args.beam_size, temperature=args.temperatures,
                                                         best_of=args.best_of, compression_ratio_threshold=args.compression_ratio_threshold,
                                                         logprob_threshold=args.logprob_threshold, no_speech_threshold=args.no_speech_threshold,
                                                         text_of=text_of, seed=args.seed)):
                for seg in res.segments:
                    ids = [t for t in seg.tokens if t < ts_begin]
                    line = f"{path}\t{seg.start:.2f}\t{seg.end:.2f}\t{' '.join(str(t) for t in ids)}"
                    if tok is not None:
                        line += "\t" + tok.decode(ids, skip_special_tokens=True).strip()
                    print(line)
            continue
        for path, n in zip(paths, lens.cpu().tolist() if hasattr(lens, "cpu") else list(lens)):
            if n > N_SAMPLES:
                raise SystemExit(f"{path}: {n / 16000:.1f} s of audio; only the first 30 s window is built (no seeking): cut the file")
        how = dict(beam_size=args.beam_size)
        if args.temperatures[0] > 0.0:  # (whisper drops the beam above temperature 0 and best_of at 0)
            how = dict(temperature=args.temperatures[0], best_of=args.best_of, seed=args.seed)
        res = model.generate(model.encode(model.features(waves, lens)), language=args.language, task=args.task,
                             max_new_tokens=args.max_new_tokens, **how)
        for path, ids in zip(paths, res.tokens):
            line = f"{path}\t{' '.join(str(t) for t in ids)}"
            if tok is not None:
                line += "\t" + tok.decode(ids, skip_special_tokens=True).strip()
            print(line)


if __name__ == "__main__":
    main()
