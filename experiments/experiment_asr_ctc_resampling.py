#!/usr/bin/env python
"""Phoneme / character recognition probe on latents RESAMPLED from a frozen latent-variable model: on every probe step, training
and evaluation alike, fresh z ~ q(z | x) are drawn for the batch, so the probe sees a new sample of the representation each epoch
(experiments/experiment_asr_ctc_resampling.py of the reference — its VRNN, SRNN, STCN and CW-VAE phoneme rows — without the wandb
lookup: the trained run is a local directory written by `save_run` / `model.save`).  The frozen model runs `model.represent`, which
launches only what the latents need; the probe, its loop and its flags are those of experiment_asr_ctc.py.  One process; the probe
runs in fp32, the frozen extractor in the process's operand mode.

  --run_dir DIR                  the trained run (model_*.pt), loaded as dump_representations.py loads it
  --z_index I                    the latent level whose z feeds the probe (0 for VRNN / SRNN)
  --num_samples K                the mean over K draws per step (default 1: one fresh draw)
  --input_coding / --num_bits    as the model was trained
  --dataset train.csv            a source CSV (`filename,length...`): `<filename>.<audio_ext>` is the waveform, `<filename>.<text_ext>`
      --text_ext EXT --tokens FILE   holds the space-separated labels, and FILE lists the tokens, one per line
  --dataset synthetic            needs no files: labelled tone waveforms and a small freshly initialised --synthetic_model
                                 (vrnn | srnn | stcn | cwvae) built from --seed.  An untrained extractor need not give a learnable
                                 representation: this is the smoke path.
"""
import sys

from _common import setup  # noqa: I001
from _asr import PROBE_DEFAULTS, SyntheticWaveforms, add_probe_flags, read_token_map, real_loaders, run_probe, synthetic_model

import torch

from blvm.data.token_map import TokenMap
from blvm.utils.argparsers import parser

parser.set_defaults(**PROBE_DEFAULTS, num_workers=12)
g = parser.add_argument_group("model")
g.add_argument("--run_dir", default=None, type=str, help="directory of the trained run whose latents are probed (model_*.pt)")
g.add_argument("--z_index", default=0, type=int, help="index of the latent representation level")
g.add_argument("--num_samples", default=1, type=int, help="draws averaged per probe step")
g.add_argument("--input_coding", default="mu_law", type=str, choices=["mu_law", "linear"], help="as the model was trained")
g.add_argument("--num_bits", default=16, type=int, help="as the model was trained")
g.add_argument("--text_type", default="phon", choices=["word", "char", "phon"], help="char: labels are characters; otherwise space-separated tokens")
g.add_argument("--text_ext", default="PHN", type=str, help="extension of the per-example label files")
g.add_argument("--tokens", default=None, type=str, help="file with one token per line (the blank is added)")
g.add_argument("--sample_rate", default=16000, type=int)
add_probe_flags(g)
g.add_argument("--synthetic_model", default="vrnn", choices=["vrnn", "srnn", "stcn", "cwvae"], help="the frozen model of --dataset synthetic")
g.add_argument("--synthetic_tokens", default=12, type=int, help="number of labels of the synthetic data")
g.add_argument("--synthetic_frames", default=120, type=int, help="longest synthetic utterance in latent frames")


def main():
    args = parser.parse_args()
    if args.use_amp:
        raise SystemExit("--use_amp True: the CTC probe runs in fp32 (the 16-bit operand modes do not cover it)")
    _, _, dev = setup(args)
    from blvm.data.transforms import LatentRepresentation

    if args.dataset == "synthetic":
        rep_model, frame_samples = synthetic_model(args.synthetic_model, args.seed)
        if not 0 <= args.z_index < len(frame_samples):
            raise SystemExit(f"--z_index {args.z_index}: the synthetic {args.synthetic_model} has {len(frame_samples)} latent level(s)")
        token_map = TokenMap([f"t{i:02d}" for i in range(args.synthetic_tokens)], add_blank=True)
        bs = args.batch_size or 16
        n_train = min(args.num_batches_per_epoch, max(args.synthetic_utterances // bs, 1))
        S = frame_samples[args.z_index]
        source = lambda n, seed: SyntheticWaveforms(n, bs, args.synthetic_tokens, args.synthetic_frames, S, seed, args.sample_rate,
                                                    pad_to=max(frame_samples))  # noqa: E731
        train, test = source(n_train, args.seed), source(max(n_train // 8, 1), args.seed + 1)
        first = next(iter(test))
    else:
        if not args.run_dir:
            raise SystemExit("--run_dir DIR (the trained run whose latents are probed) is required with a real dataset")
        from blvm.data.batchers import DynamicTensorBatcher
        from blvm.data.loaders import AudioLoader
        from blvm.data.transforms import Compose, MuLawEncode
        from blvm.training.restore import load_run

        rep_model, _ = load_run(args.run_dir, device=dev, raise_errors=False)
        token_map = read_token_map(args)
        enc = [MuLawEncode(args.num_bits)] if args.input_coding == "mu_law" else []
        train, test = real_loaders(args, token_map, features=(AudioLoader(args.audio_ext), Compose(*enc), DynamicTensorBatcher()))
        first = next(iter(test))[0]
    front_end = LatentRepresentation(rep_model.to(dev), level=args.z_index, num_samples=args.num_samples)
    (x, x_sl), _ = first
    input_size = front_end(x.to(dev), x_sl)[0].size(1)  # the level's latent size, as the reference reads it off a first batch
    return run_probe(args, dev, token_map, train, test, input_size, front_end, unwrap=args.dataset != "synthetic")


if __name__ == "__main__":
    main()
    sys.exit(0)
