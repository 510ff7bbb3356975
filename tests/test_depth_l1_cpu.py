"""CPU: the exact L1 scale-and-shift alignment on the host (harness.metrics.l1_fit / l1_objective, depth_alignment: l1)
against an independent LP solver, against the reference's lad / lad2 results in tests/golden/depth_l1_golden.npz
(make_depth_l1_golden.py), and on degenerate inputs."""
import math
import os

import numpy as np
import pytest
import torch
from scipy.optimize import linprog

from unigeo_amd.harness import SyntheticGeometryDataset, depth_evaluation, evaluate, parse_depth_coord
from unigeo_amd.harness.eval import parse_depth_eval_config
from unigeo_amd.harness.metrics import L1_MAX_STEPS, _l1_quantise, _l1_step, _l1_vertex_holds, l1_fit, l1_objective

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(GOLD, "depth_l1_golden.npz"))
A = np.load(os.path.join(GOLD, "depth_alignment_golden.npz"))
KEYS = [str(k) for k in G["keys"]]
CLIPS = dict(zip(("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max"), (float(v) for v in G["clips"])))
KINDS = ("heavy", "levels8", "integer", "gauss")


def problem(kind, seed):
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    n = int(rng.integers(2, 200))
    if kind == "heavy":
        p = rng.standard_cauchy(n)
        g = 0.7 * p + 0.3 + 0.2 * rng.standard_cauchy(n)
    elif kind == "levels8":
        p = 0.5 + 0.5 * rng.integers(0, 8, n)
        g = 0.7 * p + 0.3 + 0.2 * rng.standard_normal(n)
    elif kind == "integer":
        p, g = rng.integers(0, 6, n).astype(np.float64), rng.integers(0, 12, n).astype(np.float64)
    else:
        p, g = rng.standard_normal(n), rng.standard_normal(n)
    return p.astype(np.float32), g.astype(np.float32)


def dequantised(p):
    q, E = _l1_quantise(p)
    return q.astype(np.float64) * math.ldexp(1.0, E - 36)


def lp_optimum(p, g):
    """min sum e_i  s.t.  -e_i <= s x_i + t - g_i <= e_i, by HiGHS."""
    x, g = dequantised(p), g.astype(np.float64)
    n = len(x)
    col = np.stack([x, np.ones(n)], 1)
    r = linprog(np.r_[0.0, 0.0, np.ones(n)], A_ub=np.block([[col, -np.eye(n)], [-col, -np.eye(n)]]), b_ub=np.r_[g, -g],
                bounds=[(None, None)] * 2 + [(0, None)] * n, method="highs")
    assert r.status == 0, r.message
    return float(r.fun)


@pytest.mark.parametrize("kind", KINDS)
def test_objective_is_the_lp_optimum(kind):
    """60 seeded problems of each kind (240 in all), n in 2 .. 199: F(l1_fit) <= LP optimum * (1 + 1e-9); the slack is the LP solver's own
    tolerance."""
    worst, most = 0.0, 0
    for seed in range(60):
        p, g = problem(kind, seed)
        s, t, info = l1_fit(p, g)
        F, opt = l1_objective(p, g, s, t), lp_optimum(p, g)
        assert info["certified"] == 1 and 1 <= info["steps"] <= L1_MAX_STEPS, (seed, info)
        assert F <= opt * (1 + 1e-9), (seed, F, opt, info)
        worst, most = max(worst, (F - opt) / opt if opt > 0 else 0.0), max(most, info["steps"])
    print(f"{kind}: worst relative gap to the LP optimum {worst:.3e}, most steps {most}")


def test_the_vertex_check_moves_the_pivot_on_an_integer_problem():
    """Among the integer problems there is one whose first vertex passes the weighted median along its own pivot's line and is still not the
    minimiser: a point on the line says no.  Without the check the descent would stop there, above the optimum."""
    found = 0
    for seed in range(60):
        p, g = problem("integer", seed)
        q, E = _l1_quantise(p)
        down, g64 = math.ldexp(1.0, E - 36), g.astype(np.float64)
        j0 = int(np.argmax(p == np.sort(p)[(len(p) - 1) // 2]))
        S, tied = _l1_step(q, g64, j0, down)
        if all(_l1_vertex_holds(q, g64, int(z), S, down) for z in tied):
            continue
        s, t, info = l1_fit(p, g)
        assert info["steps"] >= 2 and info["certified"] == 1
        assert l1_objective(p, g, s, t) < l1_objective(p, g, S, float(g64[j0]) - S * (float(q[j0]) * down))
        found += 1
    assert found >= 1


def masked(tag, clip):
    pred, gt = A[f"{tag}_pred"], A[f"{tag}_gt"]
    m1 = (gt > 0) & (gt < 80)
    p = pred[m1]
    if clip:
        p = np.minimum(np.maximum(p, np.float32(CLIPS["pre_clip_min"])), np.float32(CLIPS["pre_clip_max"]))
    return p, gt[m1]


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("tag", ["a", "q", "e"])
def test_objective_is_at_most_the_reference_solvers(tag, clip):
    """A theorem, so no tolerance: the exact minimum is at most the objective at the (s, t) of the reference's BFGS (lad) and Adam (lad2)."""
    p, g = masked(tag, clip)
    s, t, info = l1_fit(p, g)
    F = l1_objective(p, g, s, t)
    assert info["certified"] == 1 and info["steps"] <= L1_MAX_STEPS
    for mode in ("lad", "lad2"):
        ref = l1_objective(p, g, *G[f"{tag}_{mode}_{'clip' if clip else 'noclip'}_st"])
        print(f"{tag} {mode}: exact {F:.9g} reference {ref:.9g}")
        assert F <= ref


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("tag", ["a", "q", "e"])
def test_metrics_within_the_reference_solvers_own_spread(tag, clip):
    """Every metric under align_with_l1 lies within |lad - lad2| (the fixture's spread, the reference's disagreement with itself) of the
    reference's lad value."""
    cname = "clip" if clip else "noclip"
    res, (s, t) = depth_evaluation(A[f"{tag}_pred"], A[f"{tag}_gt"], custom_mask=A[f"{tag}_mask"], align_with_l1=True, **(CLIPS if clip else {}))
    lad, spread = G[f"{tag}_lad_{cname}_vals"], G[f"{tag}_{cname}_spread"]
    assert res["valid_pixels"] == int(lad[8])
    for i, k in enumerate(KEYS[:8]):
        print(f"{tag}_{cname} {k:16s} l1 {res[k]:.9g} lad {lad[i]:.9g} distance {abs(res[k] - lad[i]):.3e} spread {spread[i]:.3e}")
        assert abs(res[k] - lad[i]) <= spread[i], k
    assert s == np.float32(s) and t == np.float32(t)                      # rounded once to float32, as least squares returns them
    print(f"{tag}_{cname} s l1 {s:.9g} lad {G[f'{tag}_lad_{cname}_st'][0]:.9g}")


def test_no_valid_pixel_and_one_pixel():
    assert l1_fit(np.zeros(0, np.float32), np.zeros(0, np.float32)) == (0.0, 0.0, {"j": -1, "k": -1, "steps": 0, "certified": 1})
    res, st = depth_evaluation(np.ones((1, 4, 4), np.float32), np.zeros((1, 4, 4), np.float32), align_with_l1=True)
    assert st == (0.0, 0.0) and res["valid_pixels"] == 0 and all(res[k] == 0 for k in KEYS[:8])
    s, t, info = l1_fit(np.float32([2.5]), np.float32([7.0]))
    assert (s, t) == (0.0, 7.0) and info == {"j": 0, "k": -1, "steps": 0, "certified": 1}


def test_two_pixels_give_the_line_through_both():
    p, g = np.float32([3.0, 1.0]), np.float32([5.0, 2.0])
    s, t, info = l1_fit(p, g)
    assert (s, t) == (1.5, 0.5) and sorted((info["j"], info["k"])) == [0, 1] and info["certified"] == 1
    assert l1_objective(p, g, s, t) == 0.0


def test_all_predictions_equal_gives_the_lower_median_of_gt():
    g = np.float32([4.0, 1.0, 3.0, 2.0])
    s, t, info = l1_fit(np.full(4, 1.25, np.float32), g)
    assert (s, t) == (0.0, 2.0) and info == {"j": 0, "k": -1, "steps": 0, "certified": 1}
    s, t, _ = l1_fit(np.zeros(4, np.float32), g)
    assert (s, t) == (0.0, 2.0)


def test_a_pre_clip_that_collapses_most_values_onto_one_bound():
    """60 % of the clamped predictions sit on the lower bound - one q with most of the points, so most pivots see them as weightless."""
    rng = np.random.default_rng(7)
    gt = rng.uniform(0.5, 6.0, 500).astype(np.float32)
    pred = (0.7 * gt + 0.3 + 0.1 * rng.standard_normal(500)).astype(np.float32)
    lo = float(np.sort(pred)[299])
    res, (s, t) = depth_evaluation(pred, gt, align_with_l1=True, pre_clip_min=lo)
    p = np.maximum(pred, np.float32(lo))
    assert (p == np.float32(lo)).sum() == 300
    s64, t64, info = l1_fit(p, gt)
    assert info["certified"] == 1 and (np.float32(s64), np.float32(t64)) == (np.float32(s), np.float32(t))
    F, opt = l1_objective(p, gt, s64, t64), lp_optimum(p, gt)
    assert F <= opt * (1 + 1e-9), (F, opt)


def test_the_caps_return_the_current_vertex_uncertified(monkeypatch):
    """Past either cap the fit still answers, with the vertex it stands on and ``certified = 0``."""
    from unigeo_amd.harness import metrics
    moved = next(pg for pg in (problem("integer", seed) for seed in range(60)) if l1_fit(*pg)[2]["steps"] >= 2)
    full = l1_fit(*moved)
    monkeypatch.setattr(metrics, "L1_MAX_STEPS", full[2]["steps"] - 1)
    s, t, info = l1_fit(*moved)
    assert info["certified"] == 0 and info["steps"] == full[2]["steps"] - 1
    assert l1_objective(*moved, s, t) > l1_objective(*moved, *full[:2])          # one vertex short of the minimiser
    monkeypatch.setattr(metrics, "L1_MAX_STEPS", full[2]["steps"])
    assert l1_fit(*moved) == full                                                  # the cap itself is within bounds
    p = np.arange(5, dtype=np.float32)
    g = 2 * p + 1                                                                  # collinear: four points tied at the first vertex
    monkeypatch.setattr(metrics, "L1_MAX_TIES", 3)
    assert l1_fit(p, g) == (2.0, 1.0, {"j": 2, "k": 0, "steps": 1, "certified": 0})
    monkeypatch.setattr(metrics, "L1_MAX_TIES", 4)
    assert l1_fit(p, g) == (2.0, 1.0, {"j": 2, "k": 0, "steps": 1, "certified": 1})


def test_same_input_same_bits():
    p, g = masked("q", False)
    a, b = l1_fit(p, g), l1_fit(p.copy(), g.copy())
    assert a == b and np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and np.float64(a[1]).tobytes() == np.float64(b[1]).tobytes()


def test_flags_and_configuration():
    p, g = A["a_pred"], A["a_gt"]
    for flag in ("align_with_lad", "align_with_lad2"):
        with pytest.raises(NotImplementedError):
            depth_evaluation(p, g, align_with_l1=True, **{flag: True})
    l1 = depth_evaluation(p, g, align_with_l1=True)
    assert depth_evaluation(p, g, align_with_l1=True, align_with_scale=True) == l1                                 # l1 comes before scale ...
    assert depth_evaluation(p, g, align_with_l1=True, align_with_lstsq=True) == depth_evaluation(p, g, align_with_lstsq=True)      # ... after lstsq
    assert depth_evaluation(p, g, align_with_l1=True, metric_scale=True) == depth_evaluation(p, g, metric_scale=True)
    assert parse_depth_eval_config({"eval_depth": {"depth_alignment": "l1"}})[0] == "l1"
    with pytest.raises(ValueError, match="depth_alignment"):
        parse_depth_eval_config({"eval_depth": {"depth_alignment": "lad"}})
    with pytest.raises(ValueError, match="global"):
        parse_depth_coord({"eval_depth": {"depth_alignment": "l1", "coord": "global"}})


class _AffineWithOutliers:
    """pred = (gt - 0.3) / 0.7 with 10 % of the pixels replaced by gross outliers (anywhere in twice the range of the prediction); keeps the
    samples it was given and what it answered."""

    def __init__(self):
        self.seen = []

    def forward(self, data):
        d = np.stack([-np.asarray(c)[2] for c in data["cam_coord"]], 0).astype(np.float32)          # OpenGL z -> OpenCV depth
        rng = np.random.default_rng(len(self.seen))
        pred = ((d - 0.3) / 0.7).astype(np.float32)
        bad = rng.uniform(size=d.shape) < 0.1
        pred[bad] = rng.uniform(0.0, 2.0 * float(pred.max()), int(bad.sum())).astype(np.float32)
        self.seen.append((data, pred))
        return {"pred_depths": torch.from_numpy(pred)}


def test_evaluate_runs_l1_end_to_end(tmp_path):
    from unigeo_amd.harness.io_utils import prepare_gt_label
    ds = SyntheticGeometryDataset(clip_length=5, clip_overlap=1, input_size=(32, 48), target_size=(32, 48), root="unused", num_frames=9)
    cfg = {"dataset": "SyntheticGeometryDataset", "root": "unused", "h": 32, "w": 48, "clip_length": 5, "clip_overlap": 1,
           "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"], "depth_alignment": "l1"}}
    model = _AffineWithOutliers()
    rows, _ = evaluate(cfg, dataset=ds, model=model, save_dir=str(tmp_path), verbose=False)
    assert len(rows) == len(ds) == len(model.seen) == 3
    for row, (data, pred) in zip(rows, model.seen):
        gt = prepare_gt_label(data)
        d, mask = gt["gt_depths"].numpy(), gt["gt_masks"].numpy()
        res, (s, t) = depth_evaluation(pred, d, custom_mask=mask, align_with_l1=True)
        assert row["Abs Rel"] == res["Abs Rel"] and row["delta < 1.25"] == res["delta < 1.25"]          # the row is the host function's
        m1 = (d > 0) & (d < 80)
        s64, t64, info = l1_fit(pred[m1], d[m1])
        assert info["certified"] == 1 and (np.float32(s64), np.float32(t64)) == (np.float32(s), np.float32(t))
        ls, lt = depth_evaluation(pred, d, custom_mask=mask, align_with_lstsq=True)[1]
        F, Fls = l1_objective(pred[m1], d[m1], s64, t64), l1_objective(pred[m1], d[m1], ls, lt)
        print(f"l1 (s, t) = ({s64:.6g}, {t64:.6g}) F = {F:.6g}; least squares ({ls:.6g}, {lt:.6g}) F = {Fls:.6g}")
        assert F <= Fls
