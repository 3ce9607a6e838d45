"""Regenerates tests/golden/hdf5_h5py_summary.hdf5: tests/test_hdf5io.py's seeded sample written by h5py itself with the
dtypes of the reference's DataStore.write_summary (DataStore.py:63-68). Needs an interpreter with h5py, numpy and pytest:
`python tests/golden/make_hdf5_golden.py`. Before writing, it checks that h5py reads a file of this project's writer
exactly as dataloader_predict.py:56-61 does, so the stored file and the writer agree at the time it was made.
"""
import os
import sys
import tempfile

import h5py
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from pepper_thesis_amd import hdf5io  # noqa: E402
from test_hdf5io import _sample  # noqa: E402

OUT = os.path.join(HERE, "hdf5_h5py_summary.hdf5")


def main():
    s = _sample()
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "ours.hdf5")
        with hdf5io.ImageStore(p, "w") as st:
            st.write_summary("chr20_100_200", s["contigs"], s["positions"], s["depths"], s["candidates"], s["freq"], s["images"])
        with h5py.File(p, "r") as f:
            g = f["summaries"]["chr20_100_200"]
            c = g["candidates"][()]
            assert sorted(g.keys()) == ["candidate_frequency", "candidates", "contigs", "depths", "images", "positions"]
            assert [x.decode() for x in g["contigs"][()]] == ["chr20"] * 7 and g["positions"][()].tolist() == s["positions"].tolist()
            assert [x[0].decode() if isinstance(x[0], bytes) else x[0] for x in c] == [x[0] for x in s["candidates"]]
            assert list(c.shape) == [7, 1]
            sd = h5py.check_string_dtype(g["candidates"].dtype)
            assert sd is not None and sd.encoding == "utf-8" and sd.length is None
            assert str(g["images"].dtype) == "int8" and g["images"].chunks is None
            assert np.array_equal(g["images"][()], s["images"])
            assert [str(g[k].dtype) for k in ("positions", "depths", "candidate_frequency")] == ["int32", "uint8", "uint8"]
    b = "summaries/chr20_100_200/"
    with h5py.File(OUT, "w") as f:
        dt = h5py.special_dtype(vlen=str)
        f[b + "contigs"] = np.array(["chr20"] * 7, dtype="S")
        f[b + "positions"] = np.array(s["positions"], dtype=np.int32)
        f[b + "depths"] = np.array(s["depths"], dtype=np.uint8)
        f[b + "candidates"] = np.array(s["candidates"], dtype=dt)
        f[b + "candidate_frequency"] = np.array(s["freq"], dtype=np.uint8)
        f[b + "images"] = np.array(s["images"], dtype=np.int8)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
