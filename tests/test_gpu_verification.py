"""Ensemble verification on the GPU: dgmr_ensemble_scores (csrc/verify.hip) against verification.ensemble_scores_reference on the same
arrays, NowcastVerifier's device accumulators and DGMR.verify_batch.  No test has a time threshold."""
import numpy as np
import pytest
import torch

from verification_recipe import SCALES, THRESHOLDS, case_with_reference, check_against_reference, make_case

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 16), (3, 32, 64), (2, 64, 32), (5, 96, 160)]


def _to_numpy(scores):
    from skillful_nowcasting_amd.verification import EnsembleScores

    torch.cuda.synchronize()
    return EnsembleScores(*(t.cpu().numpy() for t in scores))


@pytest.mark.parametrize("kind", ["continuous", "radar"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("m", [1, 2, 6, 32])
def test_scores_match_the_reference(m, shape, kind):
    """Counts exactly; the float64 sums within gamma * reference (verification_recipe.check_against_reference); avg and max rows
    bit-equal at scale 1.  The observation has scattered negatives / NaN / -inf, one missing 16 x 16 cell and (N > 1) one missing plane."""
    from skillful_nowcasting_amd.verification import ensemble_scores

    f, o, ref = case_with_reference(m, *shape, kind)
    got = _to_numpy(ensemble_scores(torch.from_numpy(f.copy()).cuda(), torch.from_numpy(o.copy()).cuda(), SCALES, THRESHOLDS))
    check_against_reference(got, ref, m, SCALES, f"M={m} {shape} {kind}")
    if shape[0] > 1:  # the all-missing plane
        assert (got.cells[-1] == 0).all() and (got.abs_err[-1] == 0.0).all() and (got.pair[-1] == 0.0).all()
        assert (got.contingency[-1] == 0).all() and (got.ranks[-1] == 0).all()


@pytest.mark.parametrize("scales", [(1, 2, 4, 8, 16), (16,), (16, 2, 1)], ids=str)
def test_other_scale_sets(scales):
    from skillful_nowcasting_amd.verification import ensemble_scores

    f, o, ref = case_with_reference(6, 5, 96, 160, "radar", scales, THRESHOLDS)
    got = _to_numpy(ensemble_scores(torch.from_numpy(f.copy()).cuda(), torch.from_numpy(o.copy()).cuda(), scales, THRESHOLDS))
    check_against_reference(got, ref, 6, scales, f"scales {scales}")


@pytest.mark.parametrize("m", [9, 13, 20, 27])
def test_member_counts_on_the_guarded_instantiations(m):
    """M > 8 runs a kernel unrolled for 12, 16, 24 or 32 members with the surplus ones switched off."""
    from skillful_nowcasting_amd.verification import ensemble_scores

    f, o, ref = case_with_reference(m, 2, 64, 32, "radar", (1, 2, 16), (0.5, 4.0))
    got = _to_numpy(ensemble_scores(torch.from_numpy(f.copy()).cuda(), torch.from_numpy(o.copy()).cuda(), (1, 2, 16), (0.5, 4.0)))
    check_against_reference(got, ref, m, (1, 2, 16), f"M={m}")


def test_no_thresholds_and_eight_thresholds():
    from skillful_nowcasting_amd.verification import ensemble_scores

    thr8 = (0.03125, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 64.0)
    for thr in ((), thr8):
        f, o, ref = case_with_reference(3, 3, 32, 64, "radar", (1, 8), thr)
        got = _to_numpy(ensemble_scores(torch.from_numpy(f.copy()).cuda(), torch.from_numpy(o.copy()).cuda(), (1, 8), thr))
        check_against_reference(got, ref, 3, (1, 8), f"K={len(thr)}")


@pytest.mark.parametrize("m", [6, 13])
def test_nan_members_are_neither_hit_nor_miss(m):
    """NaN in a forecast (not screened): such a member reaches no threshold and stays below none, lies neither below nor level with
    the observation.  NaNs over wet, dry and missing pixels of plane 0 only: all counts equal the reference's exactly, plane 0's sums
    are NaN where the reference's are, and the other planes keep their bound."""
    from skillful_nowcasting_amd.verification import EnsembleScores, ensemble_scores, ensemble_scores_reference

    f, o = make_case(m, 3, 32, 64, "radar", seed=7)
    rng = np.random.Generator(np.random.PCG64(70 + m))
    hole = rng.random(f[:, 0].shape) < 0.05
    hole[m // 2] |= o[0] >= 4.0  # one member NaN over every pixel that is wet at the two upper thresholds
    f[:, 0][hole] = np.nan
    thr = (0.03125, 4.0, 8.0)
    ref = ensemble_scores_reference(f, o, SCALES, thr)
    wet = ((o[0] >= 0) & (o[0] >= np.float32(4.0))).sum()
    assert wet > 0 and ref.contingency[0, 1, m // 2, :2].sum() == 0 and (ref.contingency[0, 1, :, :2].sum(axis=1) <= wet).all()
    got = _to_numpy(ensemble_scores(torch.from_numpy(f).cuda(), torch.from_numpy(o).cuda(), SCALES, thr))
    assert np.array_equal(got.cells, ref.cells) and np.array_equal(got.contingency, ref.contingency) and np.array_equal(got.ranks, ref.ranks)
    for name in ("abs_err", "pair"):
        g, r = getattr(got, name), getattr(ref, name)
        assert np.isnan(r[0]).any() and np.array_equal(np.isnan(g), np.isnan(r)), name
    rest = lambda s: EnsembleScores(*(a[1:] for a in s))  # noqa: E731
    check_against_reference(rest(got), rest(ref), m, SCALES, f"NaN members, M={m}, planes 1 and 2")


def test_strided_forecast_gives_the_bits_of_its_copy():
    """`full[:, 1]` of an [M, 3, N, H, W] tensor is read in place through the member stride."""
    from skillful_nowcasting_amd.verification import _planes_contiguous, ensemble_scores

    f, o, _ = case_with_reference(6, 3, 32, 64, "radar")
    g = torch.Generator().manual_seed(0)
    full = torch.rand(6, 3, 3, 32, 64, generator=g).cuda()
    full[:, 1] = torch.from_numpy(f.copy()).cuda()
    view = full[:, 1]
    assert not view.is_contiguous() and _planes_contiguous(view)
    obs = torch.from_numpy(o.copy()).cuda()
    a, b = ensemble_scores(view, obs), ensemble_scores(view.contiguous(), obs)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    # planes left unflattened, and a layout that has to be copied (members innermost), give the same again
    c = ensemble_scores(view.view(6, 3, 1, 32, 64), obs.view(3, 1, 32, 64))
    d = ensemble_scores(view.permute(1, 2, 3, 0).contiguous().permute(3, 0, 1, 2), obs)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a, c)) and all(torch.equal(u, v) for u, v in zip(a, d))


def test_two_runs_are_bit_identical():
    from skillful_nowcasting_amd.verification import ensemble_scores

    f, o, _ = case_with_reference(6, 5, 96, 160, "continuous")
    fc, ob = torch.from_numpy(f.copy()).cuda(), torch.from_numpy(o.copy()).cuda()
    a = [t.clone() for t in ensemble_scores(fc, ob)]
    b = ensemble_scores(fc, ob)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_out_buffers_are_filled_and_their_surroundings_untouched():
    from skillful_nowcasting_amd.verification import EnsembleScores, _out_shapes, ensemble_scores

    f, o, ref = case_with_reference(6, 3, 32, 64, "radar")
    guard = 64
    flats, outs = [], []
    for shape, dtype in _out_shapes(3, 6, len(SCALES), len(THRESHOLDS)):
        n = int(np.prod(shape))
        flat = torch.full((n + 2 * guard,), -7, dtype=dtype, device="cuda")
        flats.append(flat)
        outs.append(flat[guard:guard + n].view(shape))
    out = EnsembleScores(*outs)
    res = ensemble_scores(torch.from_numpy(f.copy()).cuda(), torch.from_numpy(o.copy()).cuda(), SCALES, THRESHOLDS, out=out)
    assert res is out
    check_against_reference(_to_numpy(out), ref, 6, SCALES, "out=")
    for flat in flats:
        assert (flat[:guard] == -7).all() and (flat[-guard:] == -7).all()
    with pytest.raises(ValueError):
        ensemble_scores(torch.from_numpy(f.copy()).cuda(), torch.from_numpy(o.copy()).cuda(), (1, 4), THRESHOLDS, out=out)


def test_runs_on_the_callers_stream():
    from skillful_nowcasting_amd.verification import ensemble_scores

    f, o, ref = case_with_reference(2, 3, 32, 64, "continuous")
    fc, ob = torch.from_numpy(f.copy()).cuda(), torch.from_numpy(o.copy()).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = ensemble_scores(fc, ob)
    side.synchronize()
    check_against_reference(type(got)(*(t.cpu().numpy() for t in got)), ref, 2, SCALES, "side stream")


def test_verifier_update_with_cases_and_weights():
    """[M, B, T, C, H, W] with weights against the reference accumulated per case on the host: the two float64 sums to the bound of the
    single planes (weights are non-negative, so it carries over to the weighted sums), the count-derived entries to 1e-15 relative."""
    from skillful_nowcasting_amd.verification import NowcastVerifier, ensemble_scores_reference

    m, b, t, c = 6, 3, 2, 2
    f, o = make_case(m, b * t * c, 32, 64, "radar", seed=11)
    o[-1] = o[1]
    w = np.array([1.0 / 0.37, 1.0 / 0.0021, 1.0])
    v = NowcastVerifier(m, t, SCALES, THRESHOLDS)
    v.update(torch.from_numpy(f.copy()).cuda().view(m, b, t, c, 32, 64), torch.from_numpy(o.copy()).cuda().view(b, t, c, 32, 64), weights=w)
    assert all(a.is_cuda and a.dtype == torch.float64 for a in v._acc)
    # one case as [M, T, C, H, W] is the same as a batch of one
    one, batch_of_one = NowcastVerifier(m, t, SCALES, THRESHOLDS), NowcastVerifier(m, t, SCALES, THRESHOLDS)
    fc, ob = torch.from_numpy(f.copy()).cuda().view(m, b, t, c, 32, 64), torch.from_numpy(o.copy()).cuda().view(b, t, c, 32, 64)
    one.update(fc[:, 1], ob[1])
    batch_of_one.update(fc[:, 1:2], ob[1:2], weights=[1.0])
    torch.cuda.synchronize()
    assert all(torch.equal(u, w_) for u, w_ in zip(one._acc, batch_of_one._acc))
    ref = ensemble_scores_reference(f, o, SCALES, THRESHOLDS)
    wc = w
    want = [(a.reshape(b, t, c, -1).astype(np.float64) * wc[:, None, None, None]).sum(axis=(0, 2)) for a in ref]
    got = [a.cpu().numpy().reshape(t, -1) for a in v._acc]
    # per scale, as in check_against_reference: the fullest plane's cells of that scale + M^2 + s^2, + b * c + 2 for the weighting and the
    # sums over cases and channels
    s2 = np.asarray([s * s for s in SCALES], dtype=np.float64)
    gamma = (ref.cells.max(axis=0) + m * m + s2 + b * c + 2) * 2.0 ** -53  # [S]
    for name, g, r in zip(ref._fields, got, want):
        gap = np.abs(g - r)
        tol = np.broadcast_to(gamma, (t, 2, len(SCALES))).reshape(t, -1) if name in ("abs_err", "pair") else 1e-15
        print(f"verifier {name}: largest relative gap {np.max(gap / np.where(r > 0, r, 1.0)):.3e}, allowed {np.min(tol):.3e} ... {np.max(tol):.3e}")
        assert (gap <= tol * r).all(), name
    res = v.compute()
    n = want[0][:, 1]
    assert np.allclose(res["crps"]["avg"][4], want[1].reshape(t, 2, 3)[:, 0, 1] / n - want[2].reshape(t, 2, 3)[:, 0, 1] / (36 * n), rtol=1e-12)


KW = dict(forecast_steps=2, output_shape=128, latent_channels=384, context_channels=192, generation_steps=2)


@pytest.fixture(scope="module")
def model_and_batch():
    import skillful_nowcasting_amd as S

    torch.manual_seed(0)
    model = S.DGMR(**KW).to("cuda")
    model.gen_ema_decay = 0.5
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 4, 1, 128, 128, generator=g).cuda()
    y = torch.rand(2, 2, 1, 128, 128, generator=g).cuda()
    y[1, 0, 0, 3:40, 5] = -1.0  # some missing observations
    return model, x, y


def _host_verifier_result(sample, y, weights):
    from skillful_nowcasting_amd.verification import NowcastVerifier

    host = NowcastVerifier(sample.shape[0], sample.shape[2], SCALES, (0.25, 0.5))
    host.update(sample.cpu(), y.cpu(), weights)
    return host


def _assert_same_metrics(dev, host, m=3, side=128):
    """The device verifier against the host one (the reference on the same sample).  Accumulators: counts exactly (the weights
    used here are small integers), the two sums within gamma * reference, per scale gamma = (n_cells + M^2 + s^2 + 8 for the
    weighting and the sum over cases) * 2^-53 with n_cells = (side / s)^2, the cells a plane can hold.  Metrics: count-derived ones
    exactly; a CRPS is a difference of two such sums, so it may differ by gamma * (abs_err / cells + pair / (M (M - 1) cells))."""
    gamma = np.asarray([(side // s) ** 2 + m * m + s * s + 8 for s in SCALES], dtype=np.float64) * 2.0 ** -53  # [S]
    d, h = [a.cpu().numpy() for a in dev._acc], [a.numpy() for a in host._acc]
    for name, g, r in zip(dev._acc._fields, d, h):
        if name in ("abs_err", "pair"):
            print(f"verify_batch {name}: largest relative gap {np.max(np.abs(g - r) / np.where(r > 0, r, 1.0)):.3e}, gamma {gamma}")
            assert (np.abs(g - r) <= gamma * r).all(), name
        else:
            assert np.array_equal(g, r), name
    a, b = dev.compute(), host.compute()
    cells, abs_err, pair = h[0], h[1], h[2]
    for pi, pool in enumerate(("avg", "max")):
        for si, s in enumerate(SCALES):
            tol = gamma[si] * (abs_err[:, pi, si] + pair[:, pi, si] / (m * (m - 1))) / cells[:, si]
            assert (np.abs(a["crps"][pool][s] - b["crps"][pool][s]) <= tol).all(), (pool, s)
            assert (np.abs(a["crps_fair"][pool][s] - b["crps_fair"][pool][s]) <= tol).all(), (pool, s)
    for t in (0.25, 0.5):
        assert np.array_equal(a["csi"][t], b["csi"][t])
    assert np.array_equal(a["csi_members"], b["csi_members"]) and np.array_equal(a["rank_histogram"], b["rank_histogram"])
    assert np.array_equal(a["cells"], b["cells"])


def test_verify_batch_scores_the_sample_it_draws(model_and_batch):
    from skillful_nowcasting_amd.verification import NowcastVerifier

    model, x, y = model_and_batch
    model.eval()
    torch.manual_seed(5)
    with torch.no_grad():
        sample = model.sample(x, 3).clone()
    assert tuple(sample.shape) == (3, 2, 2, 1, 128, 128)
    dev = NowcastVerifier(3, 2, SCALES, (0.25, 0.5))
    torch.manual_seed(5)
    out = model.verify_batch((x, y), dev, num_samples=3, weights=[2.0, 5.0])
    assert torch.equal(out, sample)
    _assert_same_metrics(dev, _host_verifier_result(sample, y, [2.0, 5.0]))


def test_verify_batch_refuses_training_mode_and_takes_the_averaged_generator(model_and_batch):
    from skillful_nowcasting_amd.verification import NowcastVerifier

    model, x, y = model_and_batch
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model.verify_batch((x, y), NowcastVerifier(3, 2), num_samples=3)
    model.training_step((x, y.clamp_min(0.0)), 0)  # one EMA training step
    model.eval()
    torch.manual_seed(6)
    with torch.no_grad():
        sample = model.sample(x, 3, use_ema=True).clone()
        torch.manual_seed(6)
        live = model.sample(x, 3).clone()
    assert not torch.equal(sample, live)
    dev = NowcastVerifier(3, 2, SCALES, (0.25, 0.5))
    torch.manual_seed(6)
    out = model.verify_batch((x, y), dev, num_samples=3, use_ema=True)
    assert torch.equal(out, sample)
    _assert_same_metrics(dev, _host_verifier_result(sample, y, None))
