"""What the two CTC probe entry points share (experiment_asr_ctc.py: features that are deterministic; experiment_asr_ctc_resampling.py:
latents drawn from a frozen model on every step): the probe's flags and defaults, the synthetic label source, the source-CSV
loaders, and the one training / evaluation loop with its printing and checkpointing.  What differs between the two — how a batch
of the first modality becomes the probe's features — is passed in as `features_of`."""
import math
import time

from _common import clip_and_step  # noqa: I001

import torch

from blvm import _hip
from blvm.data.token_map import char_tokenizer, word_tokenizer
from blvm.evaluation import Tracker
from blvm.models import SimpleLSTMASR
from blvm.utils.argparsers import str2bool

PROBE_DEFAULTS = dict(epochs=40, batch_len=120.0, optimizer="Adam", lr=3e-4, lr_scheduler="MultiStepLR",
                      lr_scheduler_kwargs=dict(milestones=[100, 200, 300], gamma=0.5), max_grad_norm=3000.0, max_grad_value=1000.0,
                      save_checkpoints=False, test_every=1)  # fmt: skip


def add_probe_flags(g):
    """The probe's own flags (the reference's names and defaults, experiments/experiment_asr_ctc.py:35-72)."""
    g.add_argument("--hidden_size", default=128, type=int, help="size of the LSTM layers")
    g.add_argument("--num_layers", default=1, type=int, help="number of LSTM layers")
    g.add_argument("--bidirectional", default=False, type=str2bool, help="bidirectional LSTM layers")
    g.add_argument("--sum_directions", default=False, type=str2bool, help="sum directions instead of concat")
    g.add_argument("--dropout_prob", default=0.30, type=float, help="dropout rate")
    g.add_argument("--temporal_dropout", default=True, type=str2bool, help="one dropout draw per feature, shared by all frames")
    g.add_argument("--num_batches_per_epoch", default=1000, type=int, help="number of batches per epoch")


class SyntheticLabelled:
    """Batches ((x [B,D,T], x_sl), (y [B,L], y_sl)): every label holds a random run of two or more frames of its own prototype vector
    plus noise, so a row has at least twice as many frames as labels and is feasible whatever its repeats."""

    def __init__(self, n_batches, batch_size, features, n_labels, max_frames, seed):
        self.n_batches, self.batch_size, self.features, self.n_labels, self.max_frames, self.seed = n_batches, batch_size, features, n_labels, max_frames, seed
        self.prototypes = torch.randn(n_labels + 1, features, generator=torch.Generator().manual_seed(seed))

    def __len__(self):
        return self.n_batches

    def label_rows(self, gen):
        """One batch's (labels, label of every frame) per row, longest first."""
        rows = []
        for _ in range(self.batch_size):
            n = int(torch.randint(1, max(self.max_frames // 6, 2), (1,), generator=gen))
            labels = torch.randint(1, self.n_labels + 1, (n,), generator=gen)
            runs = torch.randint(2, 6, (n,), generator=gen)
            rows.append((labels, torch.repeat_interleave(labels, runs)))
        rows.sort(key=lambda r: len(r[1]), reverse=True)
        return rows

    def __iter__(self):
        for i in range(self.n_batches):
            gen = torch.Generator().manual_seed(self.seed * 7919 + i)
            rows = self.label_rows(gen)
            T, L = len(rows[0][1]), max(len(r[0]) for r in rows)
            x, y = torch.zeros(len(rows), self.features, T), torch.zeros(len(rows), L, dtype=torch.long)
            for b, (labels, frames) in enumerate(rows):
                x[b, :, : len(frames)] = (self.prototypes[frames] + 0.5 * torch.randn(len(frames), self.features, generator=gen)).T
                y[b, : len(labels)] = labels
            yield (x, torch.tensor([len(r[1]) for r in rows])), (y, torch.tensor([len(r[0]) for r in rows]))


def synthetic_model(kind: str, seed: int):
    """A small, freshly initialised model of `kind` (every width a multiple of 16) -> (model, samples per latent frame by level)."""
    from blvm.models import CWVAEAudio, SRNNAudio, STCN, VRNNAudio

    torch.manual_seed(seed)
    if kind == "vrnn":
        return VRNNAudio(likelihood="DMoL", input_size=16, hidden_size=32, latent_size=16, residual_posterior=True), [16]
    if kind == "srnn":
        return SRNNAudio(likelihood="DMoL", input_size=16, hidden_size=32, latent_size=16, residual_posterior=True), [16]
    if kind == "stcn":
        return STCN(likelihood="DMoL", n_layers=3, latent_size=[16, 16, 32], res_channels=16, n_stack_frames=8), [8, 8, 8]
    if kind == "cwvae":
        return CWVAEAudio(z_size=[32, 16, 16], h_size=16, strides=[4, 2, 2], num_level_layers=2, stride_per_layer=2, likelihood="DMoL",
                          num_mix=10, num_bins=2**16, precision_posterior=True), [4, 8, 16]  # fmt: skip
    raise ValueError(f"unknown synthetic model {kind!r}")


class SyntheticWaveforms(SyntheticLabelled):
    """Batches ((x [B,L] waveforms in (-1,1), x_sl in samples), (y [B,Lmax], y_sl)): the label rows of `SyntheticLabelled`, every
    latent frame `frame_samples` samples of a tone whose frequency belongs to the frame's label, plus noise.  Every label holds two or
    more latent frames, so a row has at least twice as many latent frames as labels and is feasible whatever its repeats.  The batch is
    zero-padded to a multiple of `pad_to` samples (a hierarchy's overall stride: the Clockwork VAE takes strideable batches only)."""

    def __init__(self, n_batches, batch_size, n_labels, max_frames, frame_samples, seed, sample_rate=16000, pad_to=1):
        super().__init__(n_batches, batch_size, 1, n_labels, max_frames, seed)
        self.frame_samples, self.sample_rate, self.pad_to = int(frame_samples), sample_rate, int(pad_to)

    def __iter__(self):
        S = self.frame_samples
        for i in range(self.n_batches):
            gen = torch.Generator().manual_seed(self.seed * 7919 + i)
            rows = self.label_rows(gen)
            T, L = len(rows[0][1]) * S, max(len(r[0]) for r in rows)
            x, y = torch.zeros(len(rows), -(-T // self.pad_to) * self.pad_to), torch.zeros(len(rows), L, dtype=torch.long)
            t = torch.arange(T, dtype=torch.float32) / self.sample_rate
            for b, (labels, frames) in enumerate(rows):
                n = len(frames) * S
                hz = 200.0 + 150.0 * torch.repeat_interleave(frames, S).float()  # the label's tone
                x[b, :n] = (0.5 * torch.sin(2 * math.pi * hz * t[:n]) + 0.05 * torch.randn(n, generator=gen)).clamp(-1, 1)
                y[b, : len(labels)] = labels
            yield (x, torch.tensor([len(r[1]) * S for r in rows])), (y, torch.tensor([len(r[0]) for r in rows]))


def real_loaders(args, token_map, features=None):
    """(train, test) DataLoaders over source CSVs: the first modality `features` = (loader, transform, batcher) — by default what
    `--data_type` names —, the second the label sequences; length-bucketed samplers, longest first."""
    from blvm.data.base_dataset import BaseDataset
    from blvm.data.batchers import DynamicTensorBatcher, TextBatcher
    from blvm.data.loaders import AudioLoader, NumpyLoader, TextLoader
    from blvm.data.samplers import LengthEvalSampler, LengthTrainSampler
    from blvm.data.transforms import Compose, EncodeInteger, StackTensor
    from blvm.modules.convenience import Permute

    if features is not None:
        pass
    elif args.data_type == "spectrogram":  # padded waveforms [B,Lmax]: main() turns each batch into log-mel features on the device
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


def read_token_map(args):
    from blvm.data.token_map import TokenMap

    if not args.tokens:
        raise SystemExit("--tokens FILE (one token per line) is required with a real dataset: the project ships no phoneme or alphabet list")
    with open(args.tokens) as f:
        return TokenMap([line.rstrip("\n") for line in f if line.strip()], add_blank=True)


def probe_step(model, features_of, x, x_sl, y, y_sl, dev):
    """One forward of the probe on a batch as the loaders give it -> (loss, metrics, outputs, feature lengths)."""
    x, x_sl = features_of(x.to(dev, non_blocking=True), x_sl)
    loss, metrics, out = model(x, x_sl, y.to(dev, non_blocking=True), y_sl)
    return loss, metrics, out, x_sl


def run_probe(args, dev, token_map, train, test, input_size, features_of, unwrap):
    """Train and evaluate SimpleLSTMASR.  `features_of(x on the device, x_sl) -> (features [B,D,T], lengths)` runs inside the step
    loop, for training and for evaluation; `unwrap`: the loaders yield (modalities, metadata) instead of the modalities."""
    model = SimpleLSTMASR(token_map=token_map, input_size=input_size, hidden_size=args.hidden_size, num_layers=args.num_layers,
                          bidirectional=args.bidirectional, sum_directions=args.sum_directions, dropout_prob=args.dropout_prob,
                          temporal_dropout=args.temporal_dropout).to(dev)  # fmt: skip
    print(model.summary(), flush=True)
    params = list(model.parameters())
    optimizer = getattr(torch.optim, args.optimizer)(params, lr=args.lr, **args.optimizer_kwargs)
    scheduler = getattr(torch.optim.lr_scheduler, args.lr_scheduler)(optimizer, **args.lr_scheduler_kwargs)

    def batches(loader):  # the synthetic sources yield the two modalities, a DataLoader (modalities, metadata)
        for item in loader:
            yield item[0] if unwrap else item

    tracker, best = Tracker(), None
    for epoch in tracker.epochs(args.epochs):
        model.train()
        t0, frames, skipped = time.time(), 0, 0
        for (x, x_sl), (y, y_sl) in tracker.steps(batches(train), source="train"):
            loss, metrics, _, x_sl = probe_step(model, features_of, x, x_sl, y, y_sl, dev)
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
                    _, metrics, out, _ = probe_step(model, features_of, x, x_sl, y, y_sl, dev)
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
