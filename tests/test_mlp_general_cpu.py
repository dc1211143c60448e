"""The toy net at any architecture, the part that needs no GPU: MLPModel is the reference's container at every case of
tests/mlp_general_refs.py (keys, shapes and per-tensor digests of tests/golden/f25_mlp_general.npz), the fp32 mirror the GPU tests
judge by equals the reference's own forward bit for bit, the refusals, the command-line flags, and the C ABI of
include/dlpm_amd_mlp.h up to dlpm_mlp_finalize (routing, tile choice, the key set with and without LayerNorm)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib, cli
import mlp_general_refs as R

ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -3, -4
LDS_LIMIT = 160 * 1024


@pytest.mark.parametrize('case', list(R.CASES))
def test_container_is_the_reference_container(case):
    """Same state_dict keys in the same order, same shapes, same default initialisation under manual_seed(1)."""
    f = golden('f25_mlp_general')
    sd = R.seeded_net(case, perturb=False).state_dict()
    assert list(sd.keys()) == [str(k) for k in f[case + '__keys']]
    assert [(list(v.shape) + [-1, -1])[:2] for v in sd.values()] == f[case + '__shapes'].tolist()
    assert [R.digest(v) for v in sd.values()] == [str(d) for d in f[case + '__sha256']]


@pytest.mark.parametrize('case', list(R.CASES))
def test_fp32_mirror_is_the_reference_forward(case):
    f = golden('f25_mlp_general')
    net = R.seeded_net(case)
    gn, skip = R.CASES[case][4], R.CASES[case][5]
    y = R.forward(net.state_dict(), torch.from_numpy(f[case + '__x']), torch.from_numpy(f[case + '__t']), gn, skip, torch.float32)
    assert np.array_equal(y.numpy(), f[case + '__y'])
    y64 = R.forward(net.state_dict(), torch.from_numpy(f[case + '__x']), torch.from_numpy(f[case + '__t']), gn, skip, torch.float64)
    assert y64.dtype == torch.float64 and R.rel_l2(y, y64) < 5e-6


@pytest.mark.parametrize('kw', [dict(nunits=1025), dict(time_emb_size=1025), dict(nfeatures=65)], ids=lambda k: next(iter(k)))
def test_over_the_caps_is_refused_at_construction(kw):
    args = dict(nfeatures=2, nblocks=1, time_emb_size=32, nunits=128)
    args.update(kw)
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        dlpm_amd.MLPModel(R.config(**args))
    at_cap = dict(args, **{k: v - 1 for k, v in kw.items()})
    assert dlpm_amd.MLPModel(R.config(**at_cap)).general


def test_options_that_stay_refused_say_why():
    def cfg(**model):
        p = R.config(2, 1, 32, 128)
        p['model'].update(model)
        return p
    for model, why in ((dict(time_emb_type='sinusoidal'), 'undefined'), (dict(time_emb_type='one_dimensional_input'), 'undefined'),
                       (dict(a_pos_emb=True), 'a_pos_emb'), (dict(learn_variance=True), 'learn_variance'),
                       (dict(dropout_rate=0.1), 'dropout'), (dict(no_a=False), 'a_t')):
        with pytest.raises(NotImplementedError, match=why):
            dlpm_amd.MLPModel(cfg(**model))
    with pytest.raises(ValueError):
        dlpm_amd.MLPModel(R.config(2, 1, 32, 128), kernel='fast')


def test_routing_property():
    shipped = dlpm_amd.MLPModel(dlpm_amd.load_config('2d_data'))
    assert not shipped.general and shipped.native_flags() == 0
    assert dlpm_amd.MLPModel(dlpm_amd.load_config('2d_data'), kernel='general').general
    for case in R.CASES:
        assert R.seeded_net(case).general, case
    assert not dlpm_amd.MLPModel(R.config(5, 0, 64, 64)).general


def test_command_line_flags_reach_the_model_config():
    ap = cli.build_parser()
    a = ap.parse_args(['--config', '2d_data', '--units', '256', '--blocks', '2', '--t_embedding_size', '48'])
    p = cli.apply_model_arguments(dlpm_amd.load_config('2d_data'), a)
    assert (p['model']['nunits'], p['model']['nblocks'], p['model']['time_emb_size']) == (256, 2, 48)
    net = dlpm_amd.init_model_by_parameter(p)
    assert (net.nunits, net.nblocks, net.time_emb_size, net.general) == (256, 2, 48, True)
    a = ap.parse_args(['--config', '2d_data'])
    q = dlpm_amd.load_config('2d_data')
    assert cli.apply_model_arguments(dlpm_amd.load_config('2d_data'), a)['model'] == q['model']
    assert 'apply_model_arguments(p, a)' in inspect.getsource(cli.main)


def test_training_refuses_a_general_net_by_name():
    net = R.seeded_net('u128')
    with pytest.raises(NotImplementedError, match='64-unit'):
        dlpm_amd.training._refuse_model(net)
    dlpm_amd.training._refuse_model(dlpm_amd.MLPModel(dlpm_amd.load_config('2d_data')))


# ------------------------------------------------------------------------------------------ the C ABI, host side
def _create(F, nu, nb, te, flags=0):
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.dlpm_mlp_create_ex(F, nu, nb, te, flags, C.byref(h))
    return rc, h


def test_create_routes_and_chooses_the_tile():
    L = _lib.lib()
    assert L.dlpm_mlp_tile_rows(None) < 0 and L.dlpm_mlp_lds_bytes(None) < 0
    for args, rows in (((2, 64, 4, 32, 0), 0), ((2, 64, 4, 64, 0), 0), ((2, 64, 4, 32, _lib.MLP_FORCE_GENERAL), 32),
                       ((2, 64, 4, 65, 0), 32), ((2, 64, 4, 32, _lib.MLP_NO_SKIP), 32), ((2, 64, 4, 32, _lib.MLP_NO_LAYERNORM), 32),
                       ((2, 128, 1, 32, 0), 32), ((2, 128, 1, 32, _lib.MLP_TILE_16), 16), ((2, 128, 1, 32, _lib.MLP_TILE_32), 32), ((1, 1024, 1, 32, 0), 32),
                       ((64, 1024, 0, 1024, 0), 16), ((1, 1, 0, 1, 0), 32)):
        rc, h = _create(*args)
        assert rc == 0, (args, L.dlpm_last_error())
        assert L.dlpm_mlp_tile_rows(h) == rows, args
        lds = L.dlpm_mlp_lds_bytes(h)
        assert (lds == 0) if rows == 0 else (0 < lds <= LDS_LIMIT), (args, lds)
        L.dlpm_mlp_destroy(h)
    # dlpm_mlp_create is create_ex without flags
    h = C.c_void_p()
    assert L.dlpm_mlp_create(2, 256, 4, 32, C.byref(h)) == 0 and L.dlpm_mlp_tile_rows(h) == 32
    L.dlpm_mlp_destroy(h)
    for args in ((2, 1025, 1, 32, 0), (2, 128, 1, 1025, 0), (65, 128, 1, 32, 0)):
        rc, h = _create(*args)
        assert rc == ERR_UNSUPPORTED and b'<=' in L.dlpm_last_error(), args
    rc, h = _create(64, 1024, 0, 1024, _lib.MLP_TILE_32)          # 32 rows of that net do not fit the LDS: said at creation
    assert rc == ERR_UNSUPPORTED and b'LDS' in L.dlpm_last_error()
    for args in ((0, 128, 1, 32, 0), (2, 0, 1, 32, 0), (2, 128, -1, 32, 0), (2, 128, 1, 0, 0), (2, 128, 1, 32, 32),
                 (2, 128, 1, 32, _lib.MLP_TILE_16 | _lib.MLP_TILE_32)):
        assert _create(*args)[0] == ERR_ARG, args


@pytest.mark.parametrize('case', ['u72', 'u80_noln'])
def test_set_param_key_set_and_missing_tensor(case):
    """With LayerNorm the whole state_dict (aliases included) is accepted; without it the group_norm keys and their aliases are
    refused; finalize names a tensor that was not set -- before anything touches the device."""
    L = _lib.lib()
    nf, nb, te, nu, gn, skip, _ = R.CASES[case]
    net = R.seeded_net(case)
    rc, h = _create(nf, nu, nb, te, net.native_flags())
    assert rc == 0
    sd = {k: v.detach().float().contiguous() for k, v in net.state_dict().items()}
    left_out = 'outblocks_mean.0.t_proj.1.weight'
    for k, v in sd.items():
        if k != left_out:
            assert L.dlpm_mlp_set_param(h, k.encode(), v.data_ptr(), v.numel()) == 0, (k, L.dlpm_last_error())
    assert L.dlpm_mlp_finalize(h) == ERR_STATE and left_out.encode() in L.dlpm_last_error()
    w = sd[left_out]
    assert L.dlpm_mlp_set_param(h, left_out.encode(), w.data_ptr(), w.numel() - 1) == ERR_ARG
    one = torch.ones(nu)
    for k in ('group_norm_in.weight', 'inblock.1.bias', 'midblocks.0.group_norm1.weight', 'midblocks.0.mlp_1.2.weight',
              'outblocks_mean.0.mlp_2.2.bias'):
        assert L.dlpm_mlp_set_param(h, k.encode(), one.data_ptr(), nu) == (0 if gn else ERR_ARG), k
    for k in ('midblocks.1.mlp_1.1.bias', 'midblocks.x.mlp_1.1.bias', 'nonsense.weight'):
        assert L.dlpm_mlp_set_param(h, k.encode(), one.data_ptr(), nu) == ERR_ARG, k
    # the training entry points answer a general handle with a message, not with a launch
    assert L.dlpm_mlp_param_floats(h) == ERR_UNSUPPORTED and b'64-unit' in L.dlpm_last_error()
    assert L.dlpm_mlp_backward_workspace_bytes(h, 4) == ERR_UNSUPPORTED
    buf = np.zeros(8, dtype=np.float32)
    p = buf.ctypes.data
    assert L.dlpm_mlp_export_params_f32(h, p, 8, None) == ERR_UNSUPPORTED
    assert L.dlpm_mlp_import_params_f32(h, p, 8, None) == ERR_UNSUPPORTED
    assert L.dlpm_mlp_backward_f32(h, p, p, p, 4, p, None, p, 1 << 20, None) == ERR_UNSUPPORTED
    assert L.dlpm_mlp_sample_steps_f32(h, p, p, p, p, 10, 4, 9, 1, 0, 0, None, None) == ERR_UNSUPPORTED
    L.dlpm_mlp_destroy(h)


@pytest.mark.parametrize('case', ['u128', 'u264_te130_plain'])
def test_checkpoint_of_a_wide_net_loads_strictly(case, tmp_path):
    """A checkpoint in the reference's format goes into a fresh net of the same architecture and into no other."""
    from dlpm_amd import checkpoint
    net = R.seeded_net(case)
    path = str(tmp_path / 'wide.pt')
    checkpoint.save_checkpoint(path, {'default': net}, epoch=3, steps=7)
    fresh = R.seeded_net(case, seed=5)
    assert checkpoint.load_into(fresh, path) == (3, 7)
    a, b = net.state_dict(), fresh.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(RuntimeError):
        checkpoint.load_into(dlpm_amd.MLPModel(dlpm_amd.load_config('2d_data')), path)
