"""Transcription with a Whisper model on the GPU, greedy or by beam search (what ssak/infer/whisper_infer.py asks of
``model.transcribe``: ``temperature = 0.0``, ``beam_size`` None or N, ``condition_on_previous_text = False``)::

    python -m ssak_amd.whisper_infer AUDIO... --model DIR [--language fr] [--task transcribe] [--max_new_tokens N] [--batch_size N]
                                     [--timestamps] [--beam_size N]

prints one line per file, ``path<TAB>ids`` (the generated token ids, space-separated, without the prompt) and, where
``transformers.WhisperTokenizer`` can be imported and ``DIR`` holds a tokenizer, ``<TAB>text``.  ``DIR`` is a
``WhisperForConditionalGeneration`` folder in the HuggingFace layout (nothing is downloaded).  Without ``--language`` the language
of each file is detected first.  Audio goes through the device ingest, Whisper's 30 s window and ``ssak_logmel_whisper``, then
:meth:`ssak_amd.whisper_seq2seq.WhisperSeq2Seq.generate`.  Audio longer than 30 s is refused by name unless ``--timestamps`` is given.

``--timestamps`` runs :meth:`ssak_amd.whisper_seq2seq.WhisperSeq2Seq.transcribe` instead -- the timestamp rules, the 30 s window
seeking through a file of any length, silent windows skipped -- and prints one line per segment,
``path<TAB>start<TAB>end<TAB>ids[<TAB>text]`` (seconds; the ids without the timestamp tokens).

``--beam_size N`` (1 to 8; the reference's ``--accurate`` is 5) decodes by beam search, with and without ``--timestamps``.
"""
from __future__ import annotations

import argparse
import os


def _tokenizer(folder: str):
    """``transformers.WhisperTokenizer`` of the model folder, or None where either is missing (the ids are the contract)."""
    if not os.path.isfile(os.path.join(folder, "vocab.json")):
        return None
    try:
        from transformers import WhisperTokenizer
    except ImportError:
        return None
    return WhisperTokenizer.from_pretrained(folder)


def main(argv=None):
    from .ingest import DeviceIngest
    from .whisper_seq2seq import N_SAMPLES, WhisperSeq2Seq
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
    args = ap.parse_args(argv)
    if args.beam_size is not None and not 1 <= args.beam_size <= 8:
        ap.error("--beam_size must lie in [1, 8]")
    if args.batch_size < 1:
        ap.error("--batch_size must be at least 1")
    if args.timestamps and args.max_new_tokens is not None:
        ap.error("--max_new_tokens does not apply with --timestamps (a window decodes up to half the decoder's positions)")
    model = WhisperSeq2Seq.from_pretrained(args.model, device=args.device)
    tok = _tokenizer(args.model)
    ingest = DeviceIngest(sample_rate=16000, device=args.device, normalize=False)
    for i in range(0, len(args.audio), args.batch_size):
        paths = args.audio[i:i + args.batch_size]
        waves, lens = ingest.load_batch([(p, None, None) for p in paths])
        if args.timestamps:
            ns = lens.cpu().tolist() if hasattr(lens, "cpu") else list(lens)
            ts_begin = model.config.no_timestamps_token_id + 1
            for path, res in zip(paths, model.transcribe([waves[b, :n] for b, n in enumerate(ns)], language=args.language, task=args.task,
                                                         batch_size=args.batch_size, beam_size=args.beam_size)):
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
        res = model.generate(model.encode(model.features(waves, lens)), language=args.language, task=args.task,
                             max_new_tokens=args.max_new_tokens, beam_size=args.beam_size)
        for path, ids in zip(paths, res.tokens):
            line = f"{path}\t{' '.join(str(t) for t in ids)}"
            if tok is not None:
                line += "\t" + tok.decode(ids, skip_special_tokens=True).strip()
            print(line)


if __name__ == "__main__":
    main()
