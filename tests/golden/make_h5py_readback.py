"""Records what h5py reads from the model file modelio.save_model writes without h5py (the h5lite writer), for
tests/test_h5lite.py::test_h5py_reads_what_we_write.  Run from the repository root with an interpreter that has h5py:

    python tests/golden/make_h5py_readback.py PYTHON_WITH_H5PY

The file is written by this interpreter (tests.test_h5lite.write_h5py_case) and read by PYTHON_WITH_H5PY; the result,
with the sha256 of the file that was read, goes to tests/golden/h5py_readback.json.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.test_h5lite import write_h5py_case  # noqa: E402

READ = """
import h5py, json, sys
f = h5py.File(sys.argv[1], 'r')
g = f['config']
k = f['lstm_1'].attrs['weight_names'][0].decode()
print(json.dumps({
    "h5py": h5py.__version__,
    "width": int(g['width'][()]), "width_shape": list(g['width'].shape), "stateful": bool(g['stateful'][()]),
    "history": json.loads(g['history'][()]),
    "mapping_dtype": str(g['mapping'].dtype), "mapping_shape": list(g['mapping'].shape),
    "layer_names": [n.decode() for n in f.attrs['layer_names']],
    "lstm_1_kernel": k, "lstm_1_kernel_3_5": float(f['lstm_1'][k][3, 5]),
}))
"""


def main(python):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "m.h5")
        write_h5py_case(out)
        res = subprocess.run([python, "-c", READ, out], capture_output=True, text=True, check=True)
        record = json.loads(res.stdout)
        with open(out, "rb") as f:
            record["sha256"] = hashlib.sha256(f.read()).hexdigest()
    with open(os.path.join(HERE, "h5py_readback.json"), "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
