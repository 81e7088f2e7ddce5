"""Language identification with a Whisper model, openai-whisper's ``detect_language`` on the GPU::

    python -m ssak_amd.whisper_lang AUDIO... --model DIR [--batch_size N]

prints one line per file, ``path<TAB>code<TAB>probability``.  ``DIR`` is a ``WhisperForConditionalGeneration`` folder in the
HuggingFace layout (nothing is downloaded).  Audio goes through the device ingest (PCM WAV of any sample rate, mixed down and
resampled to 16 kHz), Whisper's 30 s window (``pad_or_trim``: shorter files are zero-padded, which covers the reference's
``audio_minimum_padding``, ssak/infer/whisper_infer.py:102-105; longer ones are cut) and ``ssak_logmel_whisper``; then the
encoder, one decoder position and the softmax over the language tokens (:meth:`ssak_amd.whisper_seq2seq.WhisperSeq2Seq.detect_language`).
No tokenizer is needed.
"""
from __future__ import annotations

import argparse


def main(argv=None):
    from .ingest import DeviceIngest
    from .whisper_seq2seq import WhisperSeq2Seq
    ap = argparse.ArgumentParser(prog="python -m ssak_amd.whisper_lang", description="Detect the spoken language of each audio file.")
    ap.add_argument("audio", nargs="+", metavar="AUDIO", help="PCM WAV file(s)")
    ap.add_argument("--model", required=True, metavar="DIR", help="Whisper model folder (HuggingFace layout)")
    ap.add_argument("--batch_size", type=int, default=8, metavar="N", help="files per batch")
    ap.add_argument("--device", default="cuda:0", help="GPU to run on")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch_size must be at least 1")
    model = WhisperSeq2Seq.from_pretrained(args.model, device=args.device)
    ingest = DeviceIngest(sample_rate=16000, device=args.device, normalize=False)
    for i in range(0, len(args.audio), args.batch_size):
        paths = args.audio[i:i + args.batch_size]
        waves, lens = ingest.load_batch([(p, None, None) for p in paths])
        codes, probs = model.detect_language(model.encode(model.features(waves, lens)))
        best = probs.max(-1).values.cpu().tolist()
        for path, code, p in zip(paths, codes, best):
            print(f"{path}\t{code}\t{p:.4f}")


if __name__ == "__main__":
    main()
