"""The weight EMA's host side: the two new entry points (exported, bound, declared; argument checks), FusedAdam's option validation,
the warm-up schedule and the model's attributes.  CPU only: the library is dlopen'ed, nothing is launched."""
import ctypes
import math
import os
import re

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import _lib

    return _lib.load()


def test_symbols_are_exported_bound_and_declared(lib):
    from conftest import ROOT
    from skillful_nowcasting_amd import _lib

    src = open(os.path.join(ROOT, "include", "dgmr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("dgmr_adam_multi_ema", 10), ("dgmr_swap_multi", 5)):
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name]) == nargs, name
        m = re.search(r"\bint %s\s*\((.*?)\);" % name, src, flags=re.S)
        assert m is not None, f"{name} is not declared in include/dgmr_hip.h"
        assert len(m.group(1).split(",")) == nargs, name
    assert lib.dgmr_abi_version() == 13  # new symbols only
    assert _lib.ADAM_DESC_DTYPE.itemsize == 56 == ctypes.sizeof(_lib.AdamDesc)


def test_entry_points_report_argument_errors_without_a_gpu(lib):
    """Null descs / ema, non-positive counts and an ema_weight outside [0, 1] (or NaN) are refused before any launch, each with
    rc != 0 and the function's name in the message."""
    buf = (ctypes.c_double * 16)()  # stands for any non-null pointer: a refused call reads nothing
    p = ctypes.cast(buf, ctypes.c_void_p)
    adam, swap = lib.dgmr_adam_multi_ema, lib.dgmr_swap_multi
    ok = (0.0, 0.999, 1e-8)
    bad_adam = [(None, p, 1, 1, *ok, 0.001, None), (p, None, 1, 1, *ok, 0.001, None), (p, p, 0, 1, *ok, 0.001, None),
                (p, p, -2, 1, *ok, 0.001, None), (p, p, 1, 0, *ok, 0.001, None), (p, p, 1, -1, *ok, 0.001, None),
                (p, p, 1, 1, *ok, -0.1, None), (p, p, 1, 1, *ok, 1.5, None), (p, p, 1, 1, *ok, float("nan"), None),
                (p, p, 1, 1, *ok, float("inf"), p), (None, p, 1, 1, *ok, 0.001, p)]
    for args in bad_adam:
        assert adam(*args, None) != 0, args
        assert b"dgmr_adam_multi_ema" in lib.dgmr_last_error(), args
    bad_swap = [(None, p, 1, 1), (p, None, 1, 1), (p, p, 0, 1), (p, p, -1, 1), (p, p, 1, 0), (p, p, 1, -3)]
    for args in bad_swap:
        assert swap(*args, None) != 0, args
        assert b"dgmr_swap_multi" in lib.dgmr_last_error(), args
    assert b"null pointer" in (adam(None, p, 1, 1, *ok, 0.5, None, None), lib.dgmr_last_error())[1]
    assert b"ema_weight" in (adam(p, p, 1, 1, *ok, 2.0, None, None), lib.dgmr_last_error())[1]


def _params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf")])
def test_ema_decay_must_lie_in_zero_one(bad):
    from skillful_nowcasting_amd.optim import FusedAdam

    with pytest.raises(ValueError, match="ema_decay"):
        FusedAdam(_params(), lr=1e-3, ema_decay=bad)
    opt = FusedAdam(_params(), lr=1e-3)
    assert opt.ema_decay is None and opt.ema_warmup is False and opt.ema_num_updates == 0
    with pytest.raises(ValueError, match="ema_decay"):
        opt.ema_decay = bad  # the option may be changed between steps: checked there too
    assert opt.ema_decay is None


@pytest.mark.parametrize("good", [0.0, 0.999])
def test_ema_decay_accepts_the_closed_open_interval(good):
    from skillful_nowcasting_amd.optim import FusedAdam

    assert FusedAdam(_params(), lr=1e-3, ema_decay=good).ema_decay == good
    opt = FusedAdam(_params(), lr=1e-3)
    opt.ema_decay = good
    assert opt.ema_decay == good and isinstance(opt.ema_decay, float)
    opt.ema_decay = None
    assert opt.ema_decay is None


def test_ema_needs_the_multi_tensor_path(monkeypatch):
    from skillful_nowcasting_amd.optim import FusedAdam

    opt = FusedAdam(_params(), lr=1e-3)
    opt.multi_tensor = False
    opt.ema_decay = 0.999
    for p in opt.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    with pytest.raises(ValueError, match="multi_tensor"):
        opt.step()  # (raised before anything touches a device: these parameters live on the host)
    monkeypatch.setattr(FusedAdam, "multi_tensor", False)
    with pytest.raises(ValueError, match="multi_tensor"):
        FusedAdam(_params(), lr=1e-3, ema_decay=0.999)


def test_ema_options_are_not_param_group_keys():
    """state_dict() stays torch.optim.Adam's: the options are attributes, the shadows live outside self.state."""
    from skillful_nowcasting_amd.optim import FusedAdam

    off = FusedAdam(_params(), lr=1e-3).state_dict()
    opt = FusedAdam(_params(), lr=1e-3, ema_decay=0.999, ema_warmup=True)
    on = opt.state_dict()
    assert set(on) == set(off)
    assert set(on["param_groups"][0]) == set(off["param_groups"][0]) == {"lr", "betas", "eps", "params"}
    assert on["state"] == off["state"] == {}
    assert opt.ema_decay == 0.999 and opt.ema_warmup is True
    ps = opt.param_groups[0]["params"]
    assert all(opt.ema(p) is None for p in ps)  # nothing has been stepped
    assert opt.ema_state_dict() == {"num_updates": 0, "shadows": {}}
    assert opt.swap_ema() == []  # nothing to exchange: no launch, no device


def test_loaded_ema_state_waits_on_the_host():
    """A state loaded while the parameters are still on the host is kept there, indexed like state_dict()["state"]."""
    from skillful_nowcasting_amd.optim import FusedAdam

    opt = FusedAdam(_params(), lr=1e-3, ema_decay=0.9)
    ps = opt.param_groups[0]["params"]
    src = {"num_updates": 7, "shadows": {1: torch.full((2, 2), 3.0)}}
    opt.load_ema_state_dict(src)
    src["shadows"][1].zero_()  # the optimiser holds a copy
    assert opt.ema_num_updates == 7
    assert opt.ema(ps[0]) is None
    assert not opt.ema(ps[1]).is_cuda and torch.equal(opt.ema(ps[1]), torch.full((2, 2), 3.0))
    out = opt.ema_state_dict()
    assert out["num_updates"] == 7 and set(out["shadows"]) == {1} and torch.equal(out["shadows"][1], torch.full((2, 2), 3.0))
    assert set(opt.state_dict()) == {"state", "param_groups"} and opt.state_dict()["state"] == {}
    with pytest.raises(ValueError, match="parameters"):
        opt.load_ema_state_dict({"num_updates": 0, "shadows": {2: torch.zeros(1)}})


def test_model_attributes_default_to_off_and_stay_out_of_hparams():
    import skillful_nowcasting_amd as S

    model = S.DGMR(forecast_steps=2, output_shape=128, latent_channels=384, context_channels=192, generation_steps=2)
    assert model.gen_ema_decay is None and model.gen_ema_warmup is False
    assert not {"gen_ema_decay", "gen_ema_warmup"} & set(dict(model.hparams))
    assert not {"gen_ema_decay", "gen_ema_warmup"} & set(getattr(model, "_hub_mixin_config", {}) or {})


@pytest.mark.parametrize("n, want", [(0, 0.1), (1, 2.0 / 11.0), (100, 101.0 / 110.0), (10 ** 6, 0.999)])
def test_warmup_schedule_is_host_arithmetic(n, want):
    """min(decay, (1 + n) / (10 + n)) with n the updates made before the step; without warm-up the decay itself."""
    from skillful_nowcasting_amd.optim import FusedAdam

    got = FusedAdam.ema_decay_at(0.999, n, True)
    assert math.isclose(got, want, rel_tol=0, abs_tol=1e-15), (n, got, want)
    assert got == min(0.999, (1 + n) / (10 + n))
    assert FusedAdam.ema_decay_at(0.999, n, False) == 0.999
    assert FusedAdam.ema_decay_at(0.05, n, True) == 0.05  # a decay below the ramp is never raised


def test_checkpoint_carries_the_generator_ema(tmp_path):
    """model.ema_state_dict() is keyed by the generator's parameter names; on_save_checkpoint stores it under "generator_ema" while
    EMA is on and load_from_checkpoint restores it (on the host: the model has not been moved to a device yet)."""
    import skillful_nowcasting_amd as S

    kw = dict(forecast_steps=2, output_shape=128, latent_channels=384, context_channels=192, generation_steps=2)
    model = S.DGMR(**kw)
    assert model.ema_state_dict() == {"num_updates": 0}  # nothing was stepped: every average is the parameter itself
    state = {n: p.detach().clone().contiguous() * 0.5 for n, p in model.generator.named_parameters()}
    state["num_updates"] = 4
    model.load_ema_state_dict(state)
    ckpt = {}
    model.on_save_checkpoint(ckpt)
    assert ckpt == {}  # EMA is off
    model.gen_ema_decay = 0.999
    model.on_save_checkpoint(ckpt)
    assert set(ckpt) == {"generator_ema"} and set(ckpt["generator_ema"]) == set(state)
    assert all(v.is_contiguous() for k, v in ckpt["generator_ema"].items() if k != "num_updates")
    path = tmp_path / "ema.ckpt"
    torch.save({"state_dict": model.state_dict(), "hyper_parameters": kw, **ckpt}, path)
    other = S.DGMR.load_from_checkpoint(str(path))
    got = other.ema_state_dict()
    assert got["num_updates"] == 4
    assert all(torch.equal(got[k], state[k]) for k in state if k != "num_updates")
    with pytest.raises(KeyError, match="unknown"):
        model.load_ema_state_dict({"num_updates": 0, "no.such.parameter": torch.zeros(1)})


def test_ema_state_loaded_before_the_optimisers_exist_reaches_every_reader():
    """Lightning calls on_load_checkpoint before the Trainer has set the optimisers up: optimizers() raises there.  The state waits, and
    the first of ema_state_dict / on_save_checkpoint / ema_scope / training_step that finds the optimiser hands it over - no reader
    sees the live weights in its place, and a save in between does not drop it."""
    import skillful_nowcasting_amd as S

    model = S.DGMR(forecast_steps=2, output_shape=128, latent_channels=384, context_channels=192, generation_steps=2)
    model.gen_ema_decay = 0.999
    state = {n: p.detach().clone().contiguous() * 0.5 for n, p in model.generator.named_parameters()}
    state["num_updates"] = 9
    real = model.optimizers

    def no_trainer():
        raise RuntimeError("DGMR is not attached to a `Trainer`.")

    model.optimizers = no_trainer
    model.on_load_checkpoint({"generator_ema": state})
    assert model._gen_ema_pending is state
    ckpt = {}
    model.on_save_checkpoint(ckpt)  # still no optimiser: the state goes out as it came in
    assert ckpt["generator_ema"] is state
    with pytest.raises(RuntimeError, match="Trainer"):
        model.ema_state_dict()  # (not swallowed: only the checkpoint hooks tolerate a missing optimiser)
    model.optimizers = real
    got = model.ema_state_dict()
    assert "_gen_ema_pending" not in model.__dict__
    assert got["num_updates"] == 9 and set(got) == set(state)
    assert all(torch.equal(got[k], state[k]) for k in state if k != "num_updates")
    ckpt = {}
    model.on_save_checkpoint(ckpt)
    assert set(ckpt["generator_ema"]) == set(state) and ckpt["generator_ema"]["num_updates"] == 9

    # the refusal inside ema_scope() is raised, not deferred
    model._in_ema_scope = True
    try:
        with pytest.raises(RuntimeError, match="ema_scope"):
            model.on_load_checkpoint({"generator_ema": state})
    finally:
        model._in_ema_scope = False
    assert "_gen_ema_pending" not in model.__dict__
