#!/usr/bin/env python
"""Phoneme / character recognition probe: SimpleLSTMASR with a CTC loss on features or on a frozen model's dumped latents — entry
point with the reference's model flags and defaults (experiments/experiment_asr_ctc.py:35-72).  One process, fp32.

  --dataset synthetic            random features with feasible random label sequences (no files needed: the smoke path)
  --dataset train.csv            a source CSV (`filename,length...`); per example `<filename>.<data_type>` holds a [T,D] array
      --data_type EXT            (.npy; the dumps of dump_representations.py are `<tag>-z0-n1.npy`); with `--data_type waveform`
      --text_ext EXT             `<filename>.<audio_ext>` is cut into frames of --hop_length samples; with `--data_type spectrogram`
      --tokens FILE              (the default: the baseline every representation is compared against) each batch of waveforms becomes
                                 log-mel features on the device (--n_fft, --win_length, --hop_length, --n_mels).
                                 `<filename>.<text_ext>` holds the space-separated labels, and FILE lists the tokens, one per line
                                 (the project ships no phoneme list)
"""
import sys

from _common import setup  # noqa: I001
from _asr import PROBE_DEFAULTS, SyntheticLabelled, add_probe_flags, read_token_map, real_loaders, run_probe  # noqa: F401

from blvm.data.token_map import TokenMap
from blvm.utils.argparsers import parser

parser.set_defaults(**PROBE_DEFAULTS)
g = parser.add_argument_group("model")
g.add_argument("--data_type", default="spectrogram", type=str, help="'waveform', 'spectrogram', or the extension of per-example [T,D] .npy files")
g.add_argument("--text_type", default="phon", choices=["word", "char", "phon"], help="char: labels are characters; otherwise space-separated tokens")
g.add_argument("--text_ext", default="PHN", type=str, help="extension of the per-example label files")
g.add_argument("--tokens", default=None, type=str, help="file with one token per line (the blank is added)")
g.add_argument("--sample_rate", default=16000, type=int)
g.add_argument("--n_fft", default=512, type=int, help="FFT size of --data_type spectrogram")
g.add_argument("--win_length", default=128, type=int, help="window size in samples of --data_type spectrogram")
g.add_argument("--hop_length", default=64, type=int, help="frame size in samples of --data_type waveform, hop of --data_type spectrogram")
g.add_argument("--n_mels", default=80, type=int, help="mel bins of --data_type spectrogram")
add_probe_flags(g)
g.add_argument("--synthetic_features", default=32, type=int, help="feature size of the synthetic data")
g.add_argument("--synthetic_tokens", default=12, type=int, help="number of labels of the synthetic data")
g.add_argument("--synthetic_frames", default=120, type=int, help="longest synthetic utterance in frames")


def main():
    args = parser.parse_args()
    if args.use_amp:
        raise SystemExit("--use_amp True: the CTC probe runs in fp32 (the 16-bit operand modes do not cover it)")
    _, _, dev = setup(args)
    front_end = None
    if args.dataset == "synthetic":
        token_map = TokenMap([f"t{i:02d}" for i in range(args.synthetic_tokens)], add_blank=True)
        bs = args.batch_size or 16
        n_train = min(args.num_batches_per_epoch, max(args.synthetic_utterances // bs, 1))
        train = SyntheticLabelled(n_train, bs, args.synthetic_features, args.synthetic_tokens, args.synthetic_frames, args.seed)
        test = SyntheticLabelled(max(n_train // 8, 1), bs, args.synthetic_features, args.synthetic_tokens, args.synthetic_frames, args.seed + 1)
        test.prototypes = train.prototypes
        input_size = args.synthetic_features
    else:
        token_map = read_token_map(args)
        train, test = real_loaders(args, token_map)
        if args.data_type == "spectrogram":
            from blvm.data.transforms import LogMelSpectrogram

            front_end = LogMelSpectrogram(args.sample_rate, args.n_fft, args.win_length, args.hop_length, args.n_mels)
            input_size = args.n_mels
        else:
            ((x, _), _), _ = next(iter(test))
            input_size = x.size(1)

    def features_of(x, x_sl):
        """The model's input from a batch on the device.  Spectrogram: the batch of waveforms becomes log-mel features there; their
        lengths 1 + samples // hop_length are monotone in the sample lengths, so the samplers' longest-first order survives."""
        if front_end is None:
            return x, x_sl
        x, _ = front_end(x, x_sl)
        return x, 1 + x_sl // args.hop_length

    return run_probe(args, dev, token_map, train, test, input_size, features_of, unwrap=args.dataset != "synthetic")


if __name__ == "__main__":
    main()
    sys.exit(0)
