"""CPU side of the class-people path: the host specification (tests/class_people_reference.py) against
scikit-learn, the properties of the planted frames that keep the GPU tests from passing vacuously, and
CrowdDensityModel's constructor validation."""
import numpy as np
import pytest

import class_people_reference as ref
from lidar_ai_recommendation_software_amd.crowd_density_model import CrowdDensityModel


@pytest.mark.parametrize("case", ref.planted_cases(), ids=str)
def test_spec_labels_equal_sklearn(case):
    from sklearn.cluster import DBSCAN
    xyz, labels = ref.planted_frames(*case)
    for eps, ms in ref.PARAMS:
        for s, x, l in zip(ref.planted_spec(*case, eps, ms), xyz, labels):
            sel = x[l == ref.PERSON].astype(np.float64)
            assert np.array_equal(s["sel"], sel)
            want = DBSCAN(eps=eps, min_samples=ms).fit(sel).labels_
            assert np.array_equal(s["lab"], want)
            inst = np.full(len(x), -1, dtype=np.int32)
            inst[l == ref.PERSON] = want
            assert np.array_equal(s["instance"], inst)


@pytest.mark.parametrize("case", ref.planted_cases(), ids=str)
@pytest.mark.parametrize("eps,ms", ref.PROPERTY_PARAMS)
def test_planted_frames_are_not_degenerate(case, eps, ms):
    """Conditions on the inputs of the GPU tests: clusters, noise, border points and a cluster scattered
    over the frame's index range in every planted frame."""
    xyz, labels = ref.planted_frames(*case)
    assert set(np.unique(labels)) == set(range(ref.CLASSES))
    for f, s in enumerate(ref.planted_spec(*case, eps, ms)):
        lab, cnt = s["lab"], s["cnt"]
        assert s["k"] >= 3, f"frame {f}: {s['k']} clusters"
        assert np.any(lab < 0), f"frame {f}: no noise point"
        assert np.any((lab >= 0) & (cnt < ms)), f"frame {f}: no border point"
        scattered = 0
        for c in range(s["k"]):
            idx = np.flatnonzero(s["instance"] == c)
            scattered += idx[-1] - idx[0] + 1 > len(idx)
        assert scattered >= 1, f"frame {f}: every cluster is contiguous in index"
        # the duplicates are there: zero distances among the selected points
        assert len(np.unique(s["sel"], axis=0)) < len(s["sel"])


@pytest.mark.parametrize("n", ref.PLANTED_SIZES)
def test_unequal_batch_sizes(n):
    xyz, labels = ref.unequal_batch(n, 5)
    want = ref.spec_batch(xyz, labels, ref.PERSON, 0.3, 5)
    assert [s["nsel"] for s in want][:3] == [0, 1, 4] and want[4]["nsel"] == n
    assert 0.25 * n < want[3]["nsel"] < 0.42 * n  # about a third
    assert [s["k"] for s in want][:3] == [0, 0, 0] and want[3]["k"] >= 3 and want[4]["k"] >= 3


def test_mostly_noise_case_still_clusters():
    # eps = 0.05: only the six-fold duplicates reach min_samples
    for s in ref.planted_spec(*ref.PLANTED_MAIN, 0.05, 5):
        assert s["k"] >= 1 and np.mean(s["lab"] < 0) > 0.5


class _Stub:
    def segment(self, xyz):
        raise AssertionError("not called")


def test_constructor_validation():
    m = CrowdDensityModel(segmenter=_Stub(), person_class=2, cluster_eps=0.4, min_samples=3)
    assert (m.person_class, m.cluster_eps, m.min_samples) == (2, 0.4, 3)
    d = CrowdDensityModel()
    assert d.segmenter is None and (d.person_class, d.cluster_eps, d.min_samples) == (1, 0.3, 5)
    with pytest.raises(ValueError):
        CrowdDensityModel(segmenter=object())
    for eps in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            CrowdDensityModel(cluster_eps=eps)
    for ms in (0, -3, 2.5):
        with pytest.raises(ValueError):
            CrowdDensityModel(min_samples=ms)
    with pytest.raises(ValueError):
        CrowdDensityModel(person_class=1.5)


def test_analyze_frames_needs_a_segmenter():
    with pytest.raises(ValueError, match="segmenter"):
        CrowdDensityModel().analyze_frames(np.zeros((1, 8, 3)))


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    from lidar_ai_recommendation_software_amd import _native as nat
    lib = nat.load_library()
    assert lib.lidar_class_people_f32(None, None, None, 1, 1, 1, 0.3, 5, 1, None, None, None, None, None, None) == -1
    assert b"lidar_class_people_f32: null pointer" in lib.lidar_last_error()
