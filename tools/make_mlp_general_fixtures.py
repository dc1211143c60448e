#!/usr/bin/env python3
"""Generate tests/golden/f25_mlp_general.npz by IMPORTING the reference, as tools/make_fixtures.py does (nothing of the reference is
copied; the file holds data only).

Run:  DLPM_REFERENCE=... PYTHONDONTWRITEBYTECODE=1 python tools/make_mlp_general_fixtures.py      (DLPM_REFERENCE = the reference checkout)

F25 general toy net   MLPModel at the architectures of tests/mlp_general_refs.py::CASES   dlpm/models/Model.py:17-211,
                                                                                           DiffusionBlocks.py:88-136
Per case <c>:
  <c>__x [16,1,F], <c>__t [16]   seeded inputs
  <c>__y [16,1,F]                the reference's MLPModel.forward, its LayerNorm weights and biases perturbed as the tests perturb them
  <c>__keys, <c>__shapes, <c>__sha256   the reference's state_dict under manual_seed(1), BEFORE the perturbation: key list, shapes
                                 (-1 padded to 2 columns) and one SHA-256 per tensor; the weights come back from the seed
For the case u128 one injected-noise trajectory of GenerativeLevyProcess.sample (T = 20, B = 8, alpha = 1.7), as f5_traj_mlp_toy_b32:
  traj__A, traj__xT, traj__z, traj__final, traj__meta
"""
import os
import sys

sys.dont_write_bytecode = True
from unittest.mock import MagicMock

import transformers  # noqa: F401  (must be imported before torchvision is stubbed: it probes for the package)
from transformers import get_scheduler  # noqa: F401

for _m in ['torchvision', 'torchvision.transforms', 'torchvision.transforms.functional',
           'torchvision.datasets', 'torchvision.datasets.utils', 'torchvision.utils', 'torchvision.models',
           'imageio', 'torchquad', 'pyemd', 'prdc', 'prd', 'prd.prd_score', 'lmdb', 'thop', 'neptune']:
    sys.modules[_m] = MagicMock()
REF = os.environ.get('DLPM_REFERENCE') or sys.exit('set DLPM_REFERENCE to the reference checkout')
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np
import torch
import yaml

from dlpm.methods.GenerativeLevyProcess import GenerativeLevyProcess
import dlpm.models.Model as ref_mlp

import mlp_general_refs as R

OUT = os.path.join(ROOT, 'tests', 'golden', 'f25_mlp_general.npz')
TRAJ_CASE, TRAJ_T, TRAJ_B, TRAJ_ALPHA = 'u128', 20, 8, 1.7
torch.set_num_threads(8)


def reference_net(case, perturb):
    nf, nb, te, nu, gn, skip, _ = R.CASES[case]
    p = yaml.safe_load(open(os.path.join(REF, 'dlpm/configs/2d_data.yml')))
    p['device'] = 'cpu'
    p['data']['nfeatures'] = nf
    p['model'].update(nblocks=nb, time_emb_size=te, nunits=nu, group_norm=gn, skip_connection=skip)
    torch.manual_seed(1)
    net = ref_mlp.MLPModel(p)
    net.eval()
    return R.perturb_norms_(net, 1) if perturb else net


class Recorder:
    """Records every torch.randn_like draw of a sample() call."""

    def __init__(self):
        self.z = []

    def __enter__(self):
        self._orig = torch.randn_like
        rec = self

        def randn_like(x, *a, **k):
            out = rec._orig(x, *a, **k)
            rec.z.append(out.clone())
            return out
        torch.randn_like = randn_like
        return self

    def __exit__(self, *a):
        torch.randn_like = self._orig


def main():
    arrs = {}
    for i, case in enumerate(R.CASES):
        nf = R.CASES[case][0]
        plain = reference_net(case, False)
        sd = plain.state_dict()
        arrs[case + '__keys'] = np.array(list(sd.keys()))
        arrs[case + '__shapes'] = np.array([(list(v.shape) + [-1, -1])[:2] for v in sd.values()], dtype=np.int64)
        arrs[case + '__sha256'] = np.array([R.digest(v) for v in sd.values()])
        net = reference_net(case, True)
        g = torch.Generator().manual_seed(2500 + i)
        x, t = torch.randn(16, 1, nf, generator=g) * 2, torch.rand(16, generator=g)
        with torch.no_grad():
            y = net(x, t)
            mirror = R.forward(net.state_dict(), x, t, R.CASES[case][4], R.CASES[case][5], torch.float32)
        assert torch.equal(y, mirror), 'the fp32 mirror of tests/mlp_general_refs.py is not the reference forward on ' + case
        arrs[case + '__x'], arrs[case + '__t'], arrs[case + '__y'] = x.numpy(), t.numpy(), y.numpy()
        print('%-20s %d tensors, |y| max %.3f' % (case, len(sd), y.abs().max()))
    net = reference_net(TRAJ_CASE, True)
    np.random.seed(0)
    torch.manual_seed(0)
    meth = GenerativeLevyProcess(alpha=TRAJ_ALPHA, device='cpu', reverse_steps=TRAJ_T, rescale_timesteps=True, isotropic=True,
                                 scale='scale_preserving', input_scaling=False)
    with Recorder() as rec, torch.no_grad():
        x, hist = meth.sample({'default': net}, [TRAJ_B, 1, 2], TRAJ_T, get_sample_history=True)
    arrs.update(traj__A=meth.dlpm.A[:, :, 0, 0].numpy(), traj__xT=hist[0].numpy(), traj__z=torch.stack(rec.z).numpy(),
                traj__final=x.numpy(), traj__meta=np.array([TRAJ_T, TRAJ_ALPHA]))
    np.savez_compressed(OUT, **arrs)
    print('wrote %s %.1f kB' % (OUT, os.path.getsize(OUT) / 1e3))


if __name__ == '__main__':
    main()
