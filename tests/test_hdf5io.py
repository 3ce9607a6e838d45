"""CPU: the image / prediction HDF5 files match the reference's format: round trip through
this module, and both directions against a file written by h5py itself with DataStore.write_summary's dtypes
(DataStore.py:63-68), stored under tests/golden/ (tests/golden/make_hdf5_golden.py)."""
import os

import numpy as np

from pepper_thesis_amd import hdf5io


def _sample(n=7):
    rng = np.random.default_rng(0)
    return dict(contigs=["chr20"] * n, positions=rng.integers(1, 1 << 30, n), depths=rng.integers(0, 126, n),
                candidates=[["1T"], ["2AGG"], ["3CAA"], ["1N"], ["2" + "A" * 60], ["3CT"], ["1G"]][:n],
                freq=rng.integers(0, 126, (n, 1)), images=rng.integers(-128, 128, (n, 33, 26)).astype(np.int8),
                probs=rng.random((n, 3)))


def test_roundtrip(tmp_path):
    s = _sample()
    p = str(tmp_path / "img.hdf5")
    with hdf5io.ImageStore(p, "w") as st:
        st.write_summary("chr20_100_200", s["contigs"], s["positions"], s["depths"], s["candidates"], s["freq"], s["images"])
        st.write_summary("chr20_200_300", s["contigs"][:2], s["positions"][:2], s["depths"][:2], s["candidates"][:2], s["freq"][:2], s["images"][:2])
    with hdf5io.ImageStore(p, "r") as st:
        assert sorted(st.summaries()) == ["chr20_100_200", "chr20_200_300"]
        r = st.read_summary("chr20_100_200")
    assert r["contigs"].dtype == np.dtype("S5") and r["contigs"].tolist() == [b"chr20"] * 7
    assert r["positions"].dtype == np.int32 and r["positions"].tolist() == s["positions"].tolist()
    assert r["depths"].dtype == np.uint8 and r["candidate_frequency"].shape == (7, 1)
    assert r["candidates"].shape == (7, 1) and r["candidates"][:, 0].tolist() == [c[0] for c in s["candidates"]]
    assert r["images"].dtype == np.int8 and np.array_equal(r["images"], s["images"])
    q = str(tmp_path / "pred.hdf")
    with hdf5io.PredictionStore(q, "w") as st:
        st.write_prediction(0, s["contigs"], s["positions"], s["depths"], s["candidates"], s["freq"], s["probs"])
    with hdf5io.PredictionStore(q, "r") as st:
        (name, b), = list(st.batches())
    assert name == "batch_0" and b["base_prediction"].dtype == np.float64 and np.array_equal(b["base_prediction"], s["probs"])


def test_interval_rules():
    from pepper_thesis_amd.make_images import downsample_indices, interval_arithmetic, split_intervals
    assert interval_arithmetic(1000, 101000) == (900, 101100, 1000, 101000)
    assert interval_arithmetic(50, 100) == (0, 200, 50, 100)
    assert split_intervals("chr20", 1, 250001) == [("chr20", 1, 100001), ("chr20", 100001, 200001), ("chr20", 200001, 250001)]
    assert downsample_indices(100).tolist() == list(range(100))
    k = downsample_indices(6000)
    assert len(k) == 5000 and len(set(k.tolist())) == 5000 and k.max() >= 5000


def _layout_and_types(path, group):
    """{dataset: (HDF5 file type id, storage layout, dims)} of one summary group, through libhdf5 itself"""
    L = hdf5io.lib()
    L.H5Dget_create_plist.restype = hdf5io.hid_t
    L.H5Dget_create_plist.argtypes = [hdf5io.hid_t]
    L.H5Pget_layout.argtypes = [hdf5io.hid_t]
    out = {}
    with hdf5io.H5File(path, "r") as f:
        for name in f.keys(group):
            did = L.H5Dopen2(f.fid, ("%s/%s" % (group, name)).encode(), hdf5io.H5P_DEFAULT)
            assert did >= 0, name
            pl = L.H5Dget_create_plist(did)
            sid = L.H5Dget_space(did)
            nd = L.H5Sget_simple_extent_ndims(sid)
            dims = (hdf5io.hsize_t * max(nd, 1))()
            L.H5Sget_simple_extent_dims(sid, dims, None)
            out[name] = (L.H5Dget_type(did), L.H5Pget_layout(pl), tuple(dims[:nd]))
            L.H5Sclose(sid)
            L.H5Pclose(pl)
            L.H5Dclose(did)
    return out


def test_against_real_h5py(tmp_path):
    """h5py's own file (tests/golden/hdf5_h5py_summary.hdf5: this module's sample written by h5py with the dtypes of
    DataStore.write_summary, DataStore.py:63-68; tests/golden/make_hdf5_golden.py) (1) has, dataset by dataset, the same
    HDF5 types (fixed-length byte strings, variable-length UTF-8 strings, int32 / uint8 / int8), storage layout
    (contiguous) and shapes as the file this module writes for the same sample, so h5py reads ours as it reads its own
    (dataloader_predict.py:56-61), and (2) is read back by this module."""
    s = _sample()
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdf5_h5py_summary.hdf5")
    g = "/summaries/chr20_100_200"
    # (1) our file, compared with h5py's
    p = str(tmp_path / "ours.hdf5")
    with hdf5io.ImageStore(p, "w") as st:
        st.write_summary("chr20_100_200", s["contigs"], s["positions"], s["depths"], s["candidates"], s["freq"], s["images"])
    ours, theirs = _layout_and_types(p, g), _layout_and_types(gold, g)
    L = hdf5io.lib()
    L.H5Tequal.argtypes = [hdf5io.hid_t, hdf5io.hid_t]
    L.H5Tget_cset.argtypes = [hdf5io.hid_t]
    L.H5Tget_strpad.argtypes = [hdf5io.hid_t]
    try:
        assert sorted(ours) == sorted(theirs) == ["candidate_frequency", "candidates", "contigs", "depths", "images", "positions"]
        for name in ours:
            a, b = ours[name][0], theirs[name][0]
            assert L.H5Tequal(a, b) > 0, name
            if L.H5Tget_class(a) == hdf5io.H5T_STRING:   # H5Tequal does not compare these
                assert (L.H5Tget_cset(a), L.H5Tget_strpad(a)) == (L.H5Tget_cset(b), L.H5Tget_strpad(b)), name
            assert ours[name][1:] == theirs[name][1:], (name, ours[name][1:], theirs[name][1:])
        cand = ours["candidates"][0]
        assert L.H5Tis_variable_str(cand) > 0 and L.H5Tget_cset(cand) == hdf5io.H5T_CSET_UTF8   # variable length UTF-8
        assert ours["candidates"][2] == (7, 1) and ours["images"][1] == 1                        # H5D_CONTIGUOUS: no chunks
    finally:
        for t in list(ours.values()) + list(theirs.values()):
            L.H5Tclose(t[0])
    with hdf5io.ImageStore(p, "r") as st:
        r = st.read_summary("chr20_100_200")
    assert r["contigs"].dtype == np.dtype("S5") and r["contigs"].tolist() == [b"chr20"] * 7
    assert r["positions"].dtype == np.int32 and r["positions"].tolist() == s["positions"].tolist()
    assert r["candidates"][:, 0].tolist() == [c[0] for c in s["candidates"]]
    assert r["images"].dtype == np.int8 and int(r["images"].astype(np.int64).sum()) == int(s["images"].astype(np.int64).sum())
    assert [r[k].dtype for k in ("positions", "depths", "candidate_frequency")] == [np.int32, np.uint8, np.uint8]
    # (2) the file written by h5py, read by this module
    with hdf5io.ImageStore(gold, "r") as st:
        r = st.read_summary("chr20_100_200")
    assert r["candidates"][:, 0].tolist() == [c[0] for c in s["candidates"]]
    assert np.array_equal(r["images"], s["images"]) and r["positions"].tolist() == s["positions"].tolist()
    assert r["contigs"].tolist() == [b"chr20"] * 7 and r["candidate_frequency"].shape == (7, 1)
