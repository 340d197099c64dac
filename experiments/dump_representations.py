#!/usr/bin/env python
"""Freeze a trained model and write its latents to disk, one array per example, for the CTC probe (experiments/
dump_representations.py of the reference, without its wandb lookup: the run is a local directory written by `save_run` /
`model.save`).

For every example of every `--sources` CSV the model runs `--num_samples` times; the mean of `output.z[i]` over the runs, cut to
`output.z_sl[i][j]` frames, is saved as `<example>.<tag>-z<i>-n<num_samples>.npy` ([T_i, Z_i] float32) next to the audio file.
`experiment_asr_ctc.py --data_type <tag>-z0-n1.npy` then trains on them.  `--dry` prints the paths and writes nothing.
"""
import argparse
import os

import _common  # noqa: F401,I001  (puts the package on the path)

import numpy as np
import torch

from blvm.training.restore import load_run
from blvm.utils.argparsers import float_or_str

parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
parser.add_argument("--run_dir", type=str, required=True, help="directory of the trained run (model_*.pt, optionally checkpoint.pt)")
parser.add_argument("--sources", type=str, nargs="+", required=True, help="source CSVs whose examples are dumped")
parser.add_argument("--tag", type=str, default="run", help="name of the run inside the file extension")
parser.add_argument("--audio_ext", type=str, default="wav")
parser.add_argument("--input_coding", type=str, default="mu_law", choices=["mu_law", "linear"], help="as the model was trained")
parser.add_argument("--num_bits", type=int, default=16, help="as the model was trained")
parser.add_argument("--num_samples", type=int, default=1, help="forward passes averaged per example")
parser.add_argument("--batch_len", type=float_or_str, default=25.0, help="batch size in samples (seconds at 16 kHz if a float)")
parser.add_argument("--seed", type=int, default=0)
parser.add_argument("--device", type=int, default=0)
parser.add_argument("--num_workers", type=int, default=8)
parser.add_argument("--dry", action="store_true", help="print what would be written, write nothing")


def whole_utterances(source, args, batch_len):
    """The evaluation half of `_common.real_data_loaders` (whole utterances, deterministic length-sorted batches, with the metadata
    that names each file).  Built here because that function also builds a training sampler, which refuses a source too small to
    fill one of its batches."""
    from blvm.data.base_dataset import BaseDataset
    from blvm.data.batchers import DynamicTensorBatcher
    from blvm.data.loaders import AudioLoader
    from blvm.data.samplers import LengthEvalSampler
    from blvm.data.transforms import Compose, MuLawEncode

    enc = [MuLawEncode(args.num_bits)] if args.input_coding == "mu_law" else []
    ds = BaseDataset(source, [(AudioLoader(args.audio_ext), Compose(*enc), DynamicTensorBatcher())])
    sampler = LengthEvalSampler(source, batch_len=batch_len)
    return torch.utils.data.DataLoader(ds, batch_sampler=sampler, collate_fn=ds.collate, num_workers=args.num_workers)


def as_levels(z, z_sl):
    """output.z / output.z_sl of a one-level model as the lists a hierarchy returns."""
    zs = [z] if torch.is_tensor(z) else list(z)
    sls = [z_sl] * len(zs) if torch.is_tensor(z_sl) else list(z_sl)
    return zs, sls


def main():
    args = parser.parse_args()
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    model, _ = load_run(args.run_dir, device=dev, raise_errors=False)
    model.eval()
    batch_len = int(16000 * args.batch_len) if isinstance(args.batch_len, float) else args.batch_len
    written = 0
    with torch.no_grad():
        for source in args.sources:
            for (x, x_sl), metadata in whole_utterances(source, args, batch_len):
                total, lens = None, None
                for _ in range(args.num_samples):
                    out = model(x.to(dev, non_blocking=True), x_sl)[2]
                    zs, lens = as_levels(out.z, out.z_sl)
                    total = [z.float() for z in zs] if total is None else [a + z.float() for a, z in zip(total, zs)]
                for j, meta in enumerate(metadata):
                    stem = os.path.splitext(meta["file"])[0]
                    for i, (z, sl) in enumerate(zip(total, lens)):
                        path = f"{stem}.{args.tag}-z{i}-n{args.num_samples}.npy"
                        if args.dry:
                            print(f"dry run: would save {path}")
                        else:
                            np.save(path, (z[j, : int(sl[j])] / args.num_samples).cpu().numpy())
                        written += 1
    print(f"{'would write' if args.dry else 'wrote'} {written} arrays")


if __name__ == "__main__":
    main()
