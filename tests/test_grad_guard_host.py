"""The gradient guard's host side: ABI 13, argument checks of the two entry points, the dgmr_grad_guard mirror and FusedAdam's
option validation.  CPU only: the library is dlopen'ed, nothing is launched."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import _lib

    return _lib.load()


def test_abi_version_is_13(lib):
    from skillful_nowcasting_amd import _lib

    assert lib.dgmr_abi_version() == 13 == _lib.ABI_VERSION


def test_entry_points_report_argument_errors_without_a_gpu(lib):
    """Null pointers, n_tensors <= 0 and total_blocks <= 0 are refused before any launch, each with rc != 0 and a message."""
    buf = (ctypes.c_double * 16)()  # stands for any non-null pointer: a refused call reads nothing
    p = ctypes.cast(buf, ctypes.c_void_p)
    norm, adam = lib.dgmr_grad_norm_multi, lib.dgmr_adam_multi_guarded
    bad_norm = [(None, 1, 1, p, p, 1.0, 0, p), (p, 1, 1, None, p, 1.0, 0, p), (p, 1, 1, p, None, 1.0, 0, p), (p, 1, 1, p, p, 1.0, 0, None),
                (p, 0, 1, p, p, 1.0, 0, p), (p, -3, 1, p, p, 1.0, 0, p), (p, 1, 0, p, p, 1.0, 0, p), (p, 1, -1, p, p, 1.0, 0, p),
                (p, 1, 1, p, p, float("nan"), 0, p)]
    for args in bad_norm:
        assert norm(*args, None) != 0, args
        assert b"dgmr_grad_norm_multi" in lib.dgmr_last_error(), args
    bad_adam = [(None, 1, 1, 0.0, 0.999, 1e-8, p), (p, 1, 1, 0.0, 0.999, 1e-8, None), (p, 0, 1, 0.0, 0.999, 1e-8, p),
                (p, -1, 1, 0.0, 0.999, 1e-8, p), (p, 1, 0, 0.0, 0.999, 1e-8, p), (p, 1, -2, 0.0, 0.999, 1e-8, p)]
    for args in bad_adam:
        assert adam(*args, None) != 0, args
        assert b"dgmr_adam_multi_guarded" in lib.dgmr_last_error(), args
    assert b"null pointer" in (norm(None, 1, 1, p, p, 1.0, 0, p, None), lib.dgmr_last_error())[1]
    assert b"null pointer" in (adam(p, 1, 1, 0.0, 0.999, 1e-8, None, None), lib.dgmr_last_error())[1]


def test_grad_guard_mirror_layout():
    """16 bytes, fields at 0 / 4 / 8 / 12, in ctypes and as the numpy record; names and order as in the header."""
    import os
    import re

    from conftest import ROOT
    from skillful_nowcasting_amd import _lib

    assert ctypes.sizeof(_lib.GradGuard) == 16 and _lib.GRAD_GUARD_DTYPE.itemsize == 16
    names = ["total_norm", "clip_coef", "skipped", "skipped_total"]
    assert [f[0] for f in _lib.GradGuard._fields_] == names
    for off, name in zip((0, 4, 8, 12), names):
        assert getattr(_lib.GradGuard, name).offset == off, name
        assert _lib.GRAD_GUARD_DTYPE.fields[name][1] == off, name
    src = open(os.path.join(ROOT, "include", "dgmr_hip.h")).read()
    m = re.search(r"typedef struct dgmr_grad_guard \{(.*?)\} dgmr_grad_guard;", src, flags=re.S)
    assert m is not None
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decls = [d.split() for d in body.split(";") if d.strip()]
    assert [d[-1] for d in decls] == names
    assert [d[0] for d in decls] == ["float", "float", "int32_t", "int32_t"]


def _params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf")])
def test_max_grad_norm_must_be_a_finite_positive_float(bad):
    from skillful_nowcasting_amd.optim import FusedAdam

    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam(_params(), lr=1e-3, max_grad_norm=bad)
    opt = FusedAdam(_params(), lr=1e-3)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.max_grad_norm = bad  # the options may be changed between steps: checked there too
    assert opt.max_grad_norm is None
    opt.max_grad_norm = 2
    assert opt.max_grad_norm == 2.0 and isinstance(opt.max_grad_norm, float)
    opt.max_grad_norm = None
    assert opt.max_grad_norm is None


@pytest.mark.parametrize("options", [dict(max_grad_norm=1.0), dict(skip_nonfinite=True)])
def test_guard_needs_the_multi_tensor_path(options, monkeypatch):
    from skillful_nowcasting_amd.optim import FusedAdam

    opt = FusedAdam(_params(), lr=1e-3)
    opt.multi_tensor = False
    for k, v in options.items():
        setattr(opt, k, v)
    with pytest.raises(ValueError, match="multi_tensor"):
        opt.step()  # (raised before anything touches a device)
    monkeypatch.setattr(FusedAdam, "multi_tensor", False)
    with pytest.raises(ValueError, match="multi_tensor"):
        FusedAdam(_params(), lr=1e-3, **options)


def test_guard_options_are_not_param_group_keys():
    """state_dict() stays interchangeable with torch.optim.Adam's: the options are attributes of the optimiser."""
    from skillful_nowcasting_amd.optim import FusedAdam

    off = FusedAdam(_params(), lr=1e-3).state_dict()
    on = FusedAdam(_params(), lr=1e-3, max_grad_norm=0.5, skip_nonfinite=True).state_dict()
    assert set(on["param_groups"][0]) == set(off["param_groups"][0]) == {"lr", "betas", "eps", "params"}
    assert set(on) == set(off)
    opt = FusedAdam(_params(), lr=1e-3, max_grad_norm=0.5, skip_nonfinite=True)
    assert opt.max_grad_norm == 0.5 and opt.skip_nonfinite is True
    assert opt.last_grad_norm is None and opt.last_clip_coef is None and opt.skipped_steps is None  # nothing has run yet
    assert opt.last_tensor_grad_norms is None and opt.last_guarded_params == [] and opt.nonfinite_parameters() == []


def test_model_attributes_default_to_off_and_stay_out_of_hparams():
    import skillful_nowcasting_amd as S

    model = S.DGMR(forecast_steps=2, output_shape=128, latent_channels=384, context_channels=192, generation_steps=2)
    assert model.gen_grad_clip_norm is None and model.disc_grad_clip_norm is None and model.skip_nonfinite_steps is False
    assert not {"gen_grad_clip_norm", "disc_grad_clip_norm", "skip_nonfinite_steps"} & set(dict(model.hparams))
