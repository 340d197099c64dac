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
import time

from _common import clip_and_step, setup  # noqa: I001

import torch

from blvm import _hip
from blvm.data.token_map import TokenMap, char_tokenizer, word_tokenizer
from blvm.evaluation import Tracker
from blvm.models import SimpleLSTMASR
from blvm.utils.argparsers import parser, str2bool

parser.set_defaults(epochs=40, batch_len=120.0, optimizer="Adam", lr=3e-4, lr_scheduler="MultiStepLR",
                    lr_scheduler_kwargs=dict(milestones=[100, 200, 300], gamma=0.5), max_grad_norm=3000.0, max_grad_value=1000.0,
                    save_checkpoints=False, test_every=1)  # fmt: skip
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
g.add_argument("--hidden_size", default=128, type=int, help="size of the LSTM layers")
g.add_argument("--num_layers", default=1, type=int, help="number of LSTM layers")
g.add_argument("--bidirectional", default=False, type=str2bool, help="bidirectional LSTM layers")
g.add_argument("--sum_directions", default=False, type=str2bool, help="sum directions instead of concat")
g.add_argument("--dropout_prob", default=0.30, type=float, help="dropout rate")
g.add_argument("--temporal_dropout", default=True, type=str2bool, help="one dropout draw per feature, shared by all frames")
g.add_argument("--num_batches_per_epoch", default=1000, type=int, help="number of batches per epoch")
g.add_argument("--synthetic_features", default=32, type=int, help="feature size of the synthetic data")
g.add_argument("--synthetic_tokens", default=12, type=int, help="number of labels of the synthetic data")
g.add_argument("--synthetic_frames", default=120, type=int, help="longest synthetic utterance in frames")


class SyntheticLabelled:
    """Batches ((x [B,D,T], x_sl), (y [B,L], y_sl)): every label holds a random run of two or more frames of its own prototype vector
    plus noise, so a row has at least twice as many frames as labels and is feasible whatever its repeats."""

    def __init__(self, n_batches, batch_size, features, n_labels, max_frames, seed):
        self.n_batches, self.batch_size, self.features, self.n_labels, self.max_frames, self.seed = n_batches, batch_size, features, n_labels, max_frames, seed
        self.prototypes = torch.randn(n_labels + 1, features, generator=torch.Generator().manual_seed(seed))

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        for i in range(self.n_batches):
            gen = torch.Generator().manual_seed(self.seed * 7919 + i)
            rows = []
            for _ in range(self.batch_size):
                n = int(torch.randint(1, max(self.max_frames // 6, 2), (1,), generator=gen))
                labels = torch.randint(1, self.n_labels + 1, (n,), generator=gen)
                runs = torch.randint(2, 6, (n,), generator=gen)
                rows.append((labels, torch.repeat_interleave(labels, runs)))
            rows.sort(key=lambda r: len(r[1]), reverse=True)
            T, L = len(rows[0][1]), max(len(r[0]) for r in rows)
            x, y = torch.zeros(len(rows), self.features, T), torch.zeros(len(rows), L, dtype=torch.long)
            for b, (labels, frames) in enumerate(rows):
                x[b, :, : len(frames)] = (self.prototypes[frames] + 0.5 * torch.randn(len(frames), self.features, generator=gen)).T
                y[b, : len(labels)] = labels
            yield (x, torch.tensor([len(r[1]) for r in rows])), (y, torch.tensor([len(r[0]) for r in rows]))


def real_loaders(args, token_map):
    from blvm.data.base_dataset import BaseDataset
    from blvm.data.batchers import DynamicTensorBatcher, TextBatcher
    from blvm.data.loaders import AudioLoader, NumpyLoader, TextLoader
    from blvm.data.samplers import LengthEvalSampler, LengthTrainSampler
    from blvm.data.transforms import Compose, EncodeInteger, StackTensor
    from blvm.modules.convenience import Permute

    if args.data_type == "spectrogram":  # padded waveforms [B,Lmax]: main() turns each batch into log-mel features on the device
        features = (AudioLoader(args.audio_ext), None, DynamicTensorBatcher())
    elif args.data_type == "waveform":
        features = (AudioLoader(args.audio_ext), Compose(StackTensor(args.hop_length), Permute(1, 0)), DynamicTensorBatcher())
    else:
        features = (NumpyLoader(args.data_type, dtype=torch.float32), Permute(1, 0), DynamicTensorBatcher())  # [T,D] -> [D,T]
    tokenizer = char_tokenizer if args.text_type == "char" else word_tokenizer
    text = (TextLoader(args.text_ext, cache=True), EncodeInteger(tokenizer, token_map), TextBatcher())
    budget = int(args.batch_len) if args.batch_len else None  # in samples of the CSV's length column (setup() converts seconds)

    def loader(source, train):
        ds = BaseDataset(source, [features, text])
        if train:
            sampler = LengthTrainSampler(source, batch_len=budget, batch_size=None if budget else args.batch_size,
                                         min_pool_size=min(512, max(len(ds) // 4, 1)), num_batches=args.num_batches_per_epoch)  # fmt: skip
        else:
            sampler = LengthEvalSampler(source, batch_len=budget, batch_size=None if budget else args.batch_size)
        return torch.utils.data.DataLoader(ds, batch_sampler=sampler, collate_fn=ds.collate, num_workers=args.num_workers)

    return loader(args.dataset, True), loader(args.test_source or args.dataset, False)


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
        if not args.tokens:
            raise SystemExit("--tokens FILE (one token per line) is required with a real dataset: the project ships no phoneme or alphabet list")
        with open(args.tokens) as f:
            token_map = TokenMap([line.rstrip("\n") for line in f if line.strip()], add_blank=True)
        train, test = real_loaders(args, token_map)
        if args.data_type == "spectrogram":
            from blvm.data.transforms import LogMelSpectrogram

            front_end = LogMelSpectrogram(args.sample_rate, args.n_fft, args.win_length, args.hop_length, args.n_mels)
            input_size = args.n_mels
        else:
            ((x, _), _), _ = next(iter(test))
            input_size = x.size(1)
    model = SimpleLSTMASR(token_map=token_map, input_size=input_size, hidden_size=args.hidden_size, num_layers=args.num_layers,
                          bidirectional=args.bidirectional, sum_directions=args.sum_directions, dropout_prob=args.dropout_prob,
                          temporal_dropout=args.temporal_dropout).to(dev)  # fmt: skip
    print(model.summary(), flush=True)
    params = list(model.parameters())
    optimizer = getattr(torch.optim, args.optimizer)(params, lr=args.lr, **args.optimizer_kwargs)
    scheduler = getattr(torch.optim.lr_scheduler, args.lr_scheduler)(optimizer, **args.lr_scheduler_kwargs)

    def batches(loader):  # the synthetic source yields the two modalities, a DataLoader (modalities, metadata)
        for item in loader:
            yield item if args.dataset == "synthetic" else item[0]

    def features_of(x, x_sl):
        """The model's input on the device.  Spectrogram: the batch of waveforms becomes log-mel features there; their lengths
        1 + samples // hop_length are monotone in the sample lengths, so the samplers' longest-first order survives."""
        x = x.to(dev, non_blocking=True)
        if front_end is None:
            return x, x_sl
        x, _ = front_end(x, x_sl)
        return x, 1 + x_sl // args.hop_length

    tracker, best = Tracker(), None
    for epoch in tracker.epochs(args.epochs):
        model.train()
        t0, frames, skipped = time.time(), 0, 0
        for (x, x_sl), (y, y_sl) in tracker.steps(batches(train), source="train"):
            x, x_sl = features_of(x, x_sl)
            loss, metrics, _ = model(x, x_sl, y.to(dev, non_blocking=True), y_sl)
            optimizer.zero_grad(set_to_none=True)
            loss.backward()
            # an infeasible row makes the loss +inf and its gradients NaN: that step is not taken
            skipped += not clip_and_step(params, optimizer, args.max_grad_value, args.max_grad_norm, skip_nonfinite=True)
            tracker.update(metrics)
            frames += int(x_sl.sum())
        scheduler.step()
        torch.cuda.synchronize()
        _hip.check_async("training epoch")
        vals = ", ".join(f"{k} {v:.4f}" for k, v in tracker.values("train").items())
        note = f" | {skipped} step(s) skipped: non-finite gradient norm" if skipped else ""
        print(f"epoch {epoch:4d} | {frames / (time.time() - t0):.3e} frames/s | {vals}{note}", flush=True)
        if (epoch - 1) % args.test_every == 0:
            model.eval()
            out = None
            with torch.no_grad():
                for (x, x_sl), (y, y_sl) in tracker.steps(batches(test), source="test"):
                    x, x_sl = features_of(x, x_sl)
                    _, metrics, out = model(x, x_sl, y.to(dev, non_blocking=True), y_sl)
                    tracker.update(metrics)
            vals = tracker.values("test")
            print("           test " + ", ".join(f"{k} {v:.4f}" for k, v in vals.items()), flush=True)
            for r, h in zip(out.refs[:2], out.hyps[:2]):
                print(f"           ref: {r}\n           hyp: {h}", flush=True)
            if best is None or vals["wer"] < best:
                best = vals["wer"]
                if args.save_checkpoints and args.checkpoint_dir:
                    model.save(args.checkpoint_dir)
        tracker.log()
    return tracker


if __name__ == "__main__":
    main()
    sys.exit(0)
