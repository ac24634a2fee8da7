"""Record the Case4 guided loop's bits on the GPU: tests/golden/dps_case4_pinned.npz.

The pin was taken at commit d562bde (the parent of the dense DPS adjoint), with that
commit's own package and library, on an MI355X:

    git worktree add /tmp/parent d562bde
    python -c 'import __graft_entry__ as g; g.build()'        # in /tmp/parent
    python tests/golden/make_pinned_case4.py /tmp/parent      # in this checkout

``confild_amd`` is imported from the directory given (default: this checkout, which
then reproduces its own bits); the fixture, the synthetic weights and the loop's
arguments are those of tests/test_gpu_dps.py::_dps_setup.  Two runs of
``p_sample_loop`` on ``dps_tiny16`` with ``Case4Operator`` and no mask:
  out_noise / dist_noise   x_start and step_noise of the fixture (one chain);
  out_seed / dist_seed     three chains from synth.normal(3, "dps/xs"), Philox seed 99.
"""
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
sys.path[:0] = [PKG, os.path.join(ROOT, "tests")]

import confild_amd  # noqa: E402  (first: the package of PKG stays the one every later import sees)

assert os.path.dirname(os.path.dirname(os.path.abspath(confild_amd.__file__))) == PKG, confild_amd.__file__
sys.path.append(ROOT)   # oracle

import numpy as np  # noqa: E402
import torch  # noqa: E402

from confild_amd import synth  # noqa: E402
from test_gpu_dps import DEV, _dps_setup  # noqa: E402


def main():
    g, model, op, cond, sampler = _dps_setup("dps_tiny16")
    y = torch.from_numpy(g["measurement"]).to(DEV)
    fn = functools.partial(cond.conditioning)
    out = sampler.p_sample_loop(model=model, x_start=torch.from_numpy(g["x_start"]).to(DEV), measurement=y,
                                measurement_cond_fn=fn, step_noise=torch.from_numpy(g["step_noise"]))
    res = dict(out_noise=out.cpu().numpy(), dist_noise=sampler.distances.cpu().numpy())
    xs = torch.from_numpy(synth.normal(3, "dps/xs", (3, 1, 16, 16))).to(DEV)
    out = sampler.p_sample_loop(model=model, x_start=xs, measurement=y, measurement_cond_fn=fn, seed=99)
    res.update(out_seed=out.cpu().numpy(), dist_seed=sampler.distances.cpu().numpy())
    path = os.path.join(HERE, "dps_case4_pinned.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, "with the package at", PKG)


if __name__ == "__main__":
    main()
