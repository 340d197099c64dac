"""No GPU: the host side of the importance-weighted bound — `ops.iw_chunks`, the two K8m symbols in the header and in the built
library, and the `--iw_samples` flag of the four latent-variable experiment scripts."""
import os
import subprocess
import sys

import pytest

from blvm import _hip, ops

from conftest import ROOT

SCRIPTS = ["experiment_vrnn_audio", "experiment_srnn_audio", "experiment_stcn_audio", "experiment_clockwork_audio"]
EXPERIMENTS = os.path.join(ROOT, "experiments")


@pytest.mark.parametrize("K", [1, 2, 4, 7, 16, 64])
@pytest.mark.parametrize("B", [1, 3, 5, 64, 200])
@pytest.mark.parametrize("max_rows", [1, 3, 12, 64, 128, 1000])
def test_iw_chunks_properties(K, B, max_rows):
    cs = ops.iw_chunks(K, B, max_rows)
    assert sum(cs) == K and all(isinstance(c, int) and c >= 1 for c in cs)
    assert all(c * B <= max_rows or c == 1 for c in cs)
    if B > max_rows:
        assert cs == [1] * K
    if K == 1:
        assert cs == [1]
    # as many particles per pass as fit: no pass but the last is smaller than the largest
    assert all(c == cs[0] for c in cs[:-1]) and cs[-1] <= cs[0]
    assert cs[0] == min(K, max(1, max_rows // B))


def test_iw_chunks_refuses_nonsense():
    for bad in ((0, 3, 12), (4, 0, 12), (4, 3, 0)):
        with pytest.raises(ValueError):
            ops.iw_chunks(*bad)


def test_symbols_declared_and_exported():
    for name, n_args in (("blvm_gauss_logratio_fwd", 14), ("blvm_iw_reduce", 6)):
        assert name in _hip.SIGNATURES, name
        assert len(_hip.SIGNATURES[name][1]) == n_args
        assert hasattr(_hip.load(), name), f"{name} is not exported by {_hip.lib_path()}"


def _script(name, *argv, code="a = e.parser.parse_args(sys.argv[1:]); print('iw_samples', a.iw_samples)"):
    """Import an experiment script (its flags register at import) in a fresh interpreter and parse `argv`."""
    prog = f"import sys; sys.path.insert(0, {EXPERIMENTS!r}); import {name} as e; {code}"
    return subprocess.run([sys.executable, "-c", prog, *argv], capture_output=True, text=True, cwd=EXPERIMENTS, timeout=120)


@pytest.mark.parametrize("name", SCRIPTS)
def test_iw_samples_flag_parses_and_defaults_to_off(name):
    p = _script(name)
    assert p.returncode == 0 and "iw_samples 0" in p.stdout, p.stderr
    p = _script(name, "--iw_samples", "16")
    assert p.returncode == 0 and "iw_samples 16" in p.stdout, p.stderr


@pytest.mark.parametrize("name", SCRIPTS)
def test_iw_samples_is_refused_with_split_eval(name):
    """The scripts themselves, as they are run: refused at the command line, before a device is touched."""
    p = subprocess.run([sys.executable, os.path.join(EXPERIMENTS, name + ".py"), "--iw_samples", "4", "--split_eval", "True"],
                       capture_output=True, text=True, cwd=EXPERIMENTS, timeout=120)  # fmt: skip
    assert p.returncode == 2, (p.returncode, p.stderr)
    assert "--iw_samples with --split_eval True" in p.stderr and "not computed over evaluation splits" in p.stderr, p.stderr
