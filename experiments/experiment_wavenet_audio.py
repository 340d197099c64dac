#!/usr/bin/env python
"""WaveNet on audio waveforms — entry point with the reference's flags (experiments/experiment_wavenet_audio.py);
no gradient clipping in this loop (:206-209)."""
from _common import run, wavenet_split_eval  # noqa: I001

from blvm.models import WaveNet
from blvm.modules.distributions import CategoricalDense, DiagonalGaussianDense, DiagonalGaussianMixtureDense, DiscretizedLogisticMixtureDense
from blvm.utils.argparsers import parser, str2bool

parser.set_defaults(lr=3e-4, epochs=3000, num_workers=8, save_checkpoints=True, optimizer="Adam")  # experiment_wavenet_audio.py:32-40
g = parser.add_argument_group("model")
g.add_argument("--n_layers", default=10, type=int)
g.add_argument("--n_stacks", default=4, type=int)
g.add_argument("--res_channels", default=64, type=int)
g.add_argument("--kernel_size", default=2, type=int)
g.add_argument("--base_dilation", default=2, type=int)
g.add_argument("--input_embedding_dim", default=1, type=int)
g.add_argument("--n_stack_frames", default=1, type=int)
g.add_argument("--generate_every", default=25, type=int)
g.add_argument("--generate_frames", default=0, type=int, help="after training: draw this many samples from a zero start (cached generation)")
g.add_argument("--input_coding", default="mu_law", type=str, choices=["mu_law", "linear"])
g.add_argument("--num_bits", default=16, type=int)
g.add_argument("--num_mix", default=10, type=int)
g.add_argument("--likelihood", default="DMoL", type=str)
g.add_argument("--random_segment_size", default=None, type=int)
g.add_argument("--split_eval", default=False, type=str2bool)

def build_model(args):
    if args.likelihood == "DMoL":
        lik = DiscretizedLogisticMixtureDense(args.res_channels, 1, num_mix=args.num_mix, num_bins=2**args.num_bits)
    elif args.likelihood == "Categorical":
        # softmax over the 2**num_bits classes (experiment_wavenet_audio.py:154-155); the model quantises its float input into the
        # targets itself ("WaveNet with the categorical head")
        lik = CategoricalDense(args.res_channels, 2**args.num_bits)
    elif args.likelihood == "Gaussian":
        lik = DiagonalGaussianDense(args.res_channels, 1, initial_sd=1, epsilon=1e-4)  # experiment_wavenet_audio.py:156-157
    elif args.likelihood[:4] == "GMM-":
        # GMM-<n> (:158-160); no input normalisation: the reference's gate for it tests "gaussian" / "gmm-" (:79), spellings its own
        # model construction rejects, so its runs never normalise ("WaveNet with the Gaussian heads")
        lik = DiagonalGaussianMixtureDense(args.res_channels, 1, num_mix=int(args.likelihood.split("-")[-1]), initial_sd=1, epsilon=1e-4)
    else:
        raise ValueError(f"Unknown likelihood: {args.likelihood}")
    # --input_embedding_dim E > 1: the class-in model, nn.Embedding(2**num_bits, E) in front of a grouped causal conv.  The reference
    # passes E as `in_channels` (:168), which its model cannot run; here it is `embedding_dim` ("WaveNet with embedded
    # input").  The float input is quantised into the classes by the model.
    embedded = dict(embedding_dim=args.input_embedding_dim, num_bins=2**args.num_bits) if args.input_embedding_dim > 1 else {}
    return WaveNet(likelihood=lik, n_layers=args.n_layers, n_stacks=args.n_stacks, res_channels=args.res_channels,
                   kernel_size=args.kernel_size, base_dilation=args.base_dilation, n_stack_frames=args.n_stack_frames, **embedded)  # fmt: skip


if __name__ == "__main__":
    args = parser.parse_args()
    model = build_model(args)
    if args.split_eval and not args.random_segment_size:
        raise SystemExit("--split_eval True needs --random_segment_size (the split length, experiment_wavenet_audio.py:226)")

    def split_eval(model, x, x_sl, tracker):  # experiment_wavenet_audio.py:224-231 (benchmarks.txt:7 runs with --split_eval True)
        wavenet_split_eval(model, x, x_sl, tracker, args.random_segment_size)

    run(args, model, lambda m, x, sl: m(x, sl), lambda m, x, sl: m(x, sl), "loss", args.num_bits, split_eval if args.split_eval else None,
        clip=False)  # fmt: skip
    if args.generate_frames > 0:
        model.eval()
        x_hat = model.generate(n_samples=1, n_frames=args.generate_frames, cached=True)
        print(f"generated {tuple(x_hat.shape)}: mean {float(x_hat.mean()):.4f}, std {float(x_hat.std()):.4f}, "
              f"{len(x_hat.unique())} distinct values", flush=True)
