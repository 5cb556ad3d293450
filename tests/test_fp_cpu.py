"""CPU tests of the feature-propagation decoder: the numpy reference restates the sequential spec, the
decoder's weight layout and its error messages, and the new entry points' argument checks (no GPU: nothing
is launched)."""
import numpy as np
import pytest

import fp_reference as ref
from lidar_ai_recommendation_software_amd import _native as nat
from lidar_ai_recommendation_software_amd import pointnet2 as pn


def _lattice(n):
    g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return (g[:n] / 4.0 - 1.0).astype(np.float32)


def _frames():
    rng = np.random.default_rng(5)
    lat = _lattice(300)
    uni = rng.uniform(-1, 1, (100, 3)).astype(np.float32)
    bad_u, bad_k = uni.copy(), uni[::3].copy()
    bad_k[3, 0] = np.nan
    bad_k[7, 1] = np.inf
    bad_u[11, 2] = np.inf
    bad_u[12, 0] = np.nan
    return {"lattice": (lat, lat[::5]), "uniform": (uni, uni[::4]), "nonfinite": (bad_u, bad_k),
            "m1": (uni, uni[:1]), "m2": (uni, uni[5:7]), "dups": (uni, np.repeat(uni[:6], 3, axis=0))}


@pytest.mark.parametrize("name", ["lattice", "uniform", "nonfinite", "m1", "m2", "dups"])
def test_vectorised_reference_equals_the_scan(name):
    u, k = _frames()[name]
    d_v, i_v = ref.three_nn_ref(u, k)
    d_s, i_s = ref.three_nn_scan(u, k)
    assert np.array_equal(d_v, d_s) and np.array_equal(i_v, i_s)
    assert d_v.dtype == np.float32 and i_v.dtype == np.int32
    if name == "lattice":  # the frame exercises the tie rule
        d = np.sort(ref.dist2(u, k), axis=1)
        assert (d[:, 2] == d[:, 3]).mean() > 0.1
    if name == "nonfinite":
        assert not np.isin(i_v[:, :], [3, 7]).any()
        assert np.array_equal(d_v[11], [np.inf] * 3) and np.array_equal(d_v[12], [np.inf] * 3)
        w = ref.weights_ref(d_v)
        assert np.isnan(w[11]).all() and np.isnan(w[12]).all() and np.isfinite(np.delete(w, [11, 12], 0)).all()


@pytest.mark.parametrize("name", ["lattice", "uniform", "nonfinite", "m1", "m2", "dups"])
def test_reference_prefilter_equals_the_full_stable_argsort(name):
    u, k = _frames()[name]
    d = ref.dist2(u, k)
    key = np.where(d < np.inf, d, np.float32(np.inf))
    order = np.argsort(key, axis=1, kind="stable")[:, :3]
    srt = np.take_along_axis(key, order, axis=1)
    want_d = np.full((len(u), 3), np.inf, np.float32)
    want_i = np.zeros((len(u), 3), np.int32)
    want_d[:, :srt.shape[1]] = srt
    want_i[:, :srt.shape[1]] = np.where(srt < np.inf, order, 0)
    got_d, got_i = ref.three_nn_ref(u, k, chunk=64)
    assert np.array_equal(got_d, want_d) and np.array_equal(got_i, want_i)


def test_weights_reference_edge_cases():
    w = ref.weights_ref(np.array([[0.25, np.inf, np.inf], [0.0, 1.0, 4.0], [np.inf] * 3], np.float32))
    assert np.array_equal(w[0], [1.0, 0.0, 0.0])  # one known point: a broadcast
    assert w[1, 0] > 0.999999 and w[1].dtype == np.float32  # a zero distance dominates, nothing divides by 0
    assert np.isnan(w[2]).all()
    f = np.arange(12, dtype=np.float32).reshape(3, 4)
    out = ref.interpolate_ref(f, np.array([[2, 0, 0]]), w[:1], skip=np.ones((1, 2), np.float32))
    assert np.array_equal(out, [[8, 9, 10, 11, 1, 1]])


@pytest.mark.parametrize("cfg", [pn.SSG, pn.MSG, pn.SA1_ONLY])
def test_fp_weight_shapes(cfg):
    fp_cfg = pn.FP_SSG if cfg is not pn.SA1_ONLY else {"mlps": [[64, 32]], "head": []}
    w = pn.init_fp_weights(cfg, fp_cfg, 5, seed=3)
    ch = pn.level_channels(cfg)
    L = len(cfg["levels"])
    assert len(w["fp"]) == L and len(w["head"]) == len(fp_cfg["head"]) + 1
    c2 = ch[L]
    for i, (layers, widths) in enumerate(zip(w["fp"], fp_cfg["mlps"])):
        assert pn.fp_input_widths(cfg, fp_cfg)[i] == (c2, ch[L - i - 1])
        cin = c2 + ch[L - i - 1]
        for (W, b), cout in zip(layers, widths):
            assert W.shape == (cin, cout) and b.shape == (cout,) and W.dtype == np.float32
            assert np.abs(W).max() <= 1 / np.sqrt(cin)
            cin = cout
        c2 = widths[-1]
    assert w["head"][-1][0].shape[1] == 5 and w["head"][0][0].shape[0] == fp_cfg["mlps"][-1][-1]
    again = pn.init_fp_weights(cfg, fp_cfg, 5, seed=3)
    assert all(np.array_equal(a, b) for x, y in zip(w["head"], again["head"]) for a, b in zip(x, y))
    checked = pn.check_fp_weights(cfg, fp_cfg, 5, w)
    assert all(np.array_equal(a, b) for x, y in zip(w["fp"][0], checked["fp"][0]) for a, b in zip(x, y))


def test_fp_ssg_widths():
    # SSG: the global vector (1024) onto the 256-channel level, then 256 + 128, then no skip at the frame
    assert pn.fp_input_widths(pn.SSG, pn.FP_SSG) == [(1024, 256), (256, 128), (128, 0)]
    assert pn.fp_input_widths(pn.MSG, pn.FP_SSG) == [(1024, 640), (256, 320), (128, 0)]


def test_check_fp_weights_names_the_mismatch():
    w = pn.init_fp_weights(pn.SSG, pn.FP_SSG, 2, 0)
    with pytest.raises(ValueError, match=r"fp_weights fp1 layer 0: W \(384, 256\).*expected \(576, 256\)"):
        pn.check_fp_weights(pn.MSG, pn.FP_SSG, 2, {"fp": [pn.init_fp_weights(pn.MSG)["fp"][0]] + w["fp"][1:],
                                                   "head": w["head"]})
    with pytest.raises(ValueError, match=r"fp_weights head layer 1: W \(128, 2\).*expected \(128, 3\)"):
        pn.check_fp_weights(pn.SSG, pn.FP_SSG, 3, w)
    with pytest.raises(ValueError, match="2 FP levels, the configuration has 3"):
        pn.check_fp_weights(pn.SSG, pn.FP_SSG, 2, {"fp": w["fp"][:2], "head": w["head"]})
    with pytest.raises(ValueError, match="fp_weights fp2: 2 layers, expected 3"):
        pn.check_fp_weights(pn.SSG, pn.FP_SSG, 2, {"fp": w["fp"][:2] + [w["fp"][2][:2]], "head": w["head"]})
    with pytest.raises(ValueError, match="keys 'fp' and 'head'"):
        pn.check_fp_weights(pn.SSG, pn.FP_SSG, 2, w["fp"])
    with pytest.raises(ValueError, match="2 FP levels, the encoder has 3 levels"):
        pn.init_fp_weights(pn.SSG, {"mlps": [[8], [8]], "head": []}, 2)


def test_fp_weights_round_trip(tmp_path):
    w = pn.init_fp_weights(pn.MSG, pn.FP_SSG, 4, seed=9)
    path = str(tmp_path / "fp.npz")
    pn.save_fp_weights(path, w)
    back = pn.load_fp_weights(path, pn.MSG, pn.FP_SSG, 4)
    for a, b in zip(w["fp"] + [w["head"]], back["fp"] + [back["head"]]):
        assert all(np.array_equal(x, y) for la, lb in zip(a, b) for x, y in zip(la, lb))
    with pytest.raises(ValueError, match="fp_weights"):
        pn.load_fp_weights(path, pn.SSG, pn.FP_SSG, 4)


def test_entry_points_reject_a_null_handle():
    lib = nat.load_library()
    assert lib.lidar_three_nn_f32(None, None, None, 1, 1, 1, None, None, None, None) == -1
    assert b"lidar_three_nn_f32: null handle" in lib.lidar_last_error()
    assert lib.lidar_three_interpolate_f32(None, None, 4, 4, None, None, None, 0, 0, 1, 1, 1, None, 128, 4, None) == -1
    assert b"lidar_three_interpolate_f32: null handle" in lib.lidar_last_error()
    assert lib.lidar_row_argmax_f32(None, None, 1, 1, 1, None, None) == -1
    assert b"lidar_row_argmax_f32: null handle" in lib.lidar_last_error()
