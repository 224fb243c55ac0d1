"""Model file I/O without h5py (ocrd_keraslm_amd/lib/h5lite.py, modelio.py).

Fixture tests/golden/ref_model.h5 was written by the REFERENCE's own `Rater.save`
(rating.py:918-945) on top of a Keras-2.3-style `save_weights` layout made with
h5py 3.3 (tests/golden/make_golden.py): incl. weightless layers in `layer_names`,
the TF-uniquified scope `lstm_1/lstm_1_1/kernel:0`, a variable-length JSON string,
numpy-bool enums and the uint32 mapping."""
import hashlib
import json
import os
import tempfile

import numpy as np

from oracle import lstm_oracle as O
from ocrd_keraslm_amd.lib import Rater, h5lite, modelio
from tests.oracle_engine import OracleLM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = os.path.join(GOLD, "ref_model.h5")
SEAM = json.load(open(os.path.join(GOLD, "rater_seam.json")))


def expected_weights():
    m = SEAM["model"]
    cfg = O.ModelConfig(m["depth"], m["width"], len(m["chars"]) + 1, 1)
    return O.init_weights(cfg, seed=m["seed"], emb_std=m["emb_std"], dtype=np.float64)


def test_reader_on_reference_written_file():
    f = h5lite.H5File(REF)
    names = [n.decode() for n in f.attrs("/")["layer_names"]]
    assert names[:5] == ["char_input", "context1_input", "char_embedding", "context1_embedding", "concat_hidden_input"]
    assert f.attrs("/")["keras_version"] in ("2.3.1", b"2.3.1")
    assert f.keys("/lstm_1") == ["lstm_1_1"]                       # never hard-code dataset names
    assert [n.decode() for n in f.attrs("/lstm_1")["weight_names"]][0] == "lstm_1_1/kernel:0"
    assert f.read("/config/width") == 32 and f.read("/config/depth") == 2 and f.read("/config/length") == 16
    assert f.read("/config/stateful") == True and f.read("/config/variable_length") == False   # noqa: E712
    assert json.loads(f.read("/config/history"))["loss"] == [3.5, 3.25]
    mapping = f.read("/config/mapping")
    assert mapping.dtype == np.uint32 and mapping[0] == 0 and "".join(chr(c) for c in mapping[1:]) == "".join(SEAM["model"]["chars"])


def test_rater_loads_reference_file_and_rates_like_the_reference():
    """load_config / configure / load_weights (rate.py:76-91) on the reference-written
    file, then `rate` must reproduce the reference's golden probabilities."""
    r = Rater(engine_factory=OracleLM)
    r.load_config(REF)
    assert (r.width, r.depth, r.length, r.stateful, r.voc_size) == (32, 2, 16, True, len(SEAM["model"]["chars"]) + 1)
    assert r.history["val_loss"] == [3.4, 3.3]
    r.configure()
    r.load_weights(REF)
    assert r.status == 2
    w, ref = r.model.get_weights(), expected_weights()
    for k in ref:
        assert np.abs(w[k] - ref[k]).max() < 1e-6, k
    r.model.reset_states(1)
    case = SEAM["rate"][0]
    probs = r.rate(case["text"], case["context"])
    assert np.abs(np.array(probs, dtype=np.float64) - np.array(case["probs"])).max() < 1e-6    # weights are f32 on disk


def test_save_roundtrip_and_keras_layout():
    with tempfile.TemporaryDirectory() as tmp:
        r = Rater(engine_factory=OracleLM)
        r.load_config(REF)
        r.configure()
        r.load_weights(REF)
        out = os.path.join(tmp, "model.h5")
        r.save(out)
        assert modelio.is_hdf5(out)
        f = h5lite.H5File(out)
        assert [n.decode() for n in f.attrs("/")["layer_names"]] == modelio.keras_layer_list(2, 1)
        assert f.read("/lstm_2/lstm_2/recurrent_kernel:0").shape == (32, 128)
        r2 = Rater(engine_factory=OracleLM)
        r2.load_config(out)
        r2.configure()
        r2.load_weights(out)
        assert r2.mapping == r.mapping and r2.history == r.history
        for k, v in r.model.get_weights().items():
            assert np.array_equal(v, r2.model.get_weights()[k]), k
        # a checkpoint carries weights only (ModelCheckpoint save_weights_only, rating.py:284-285)
        ck = os.path.join(tmp, "ckpt.01-3.40.h5")
        modelio.save_weights(ck, r.model.get_weights(), 2, 1)
        assert "config" not in h5lite.H5File(ck).keys("/")
        w = modelio.load_weights(ck, 2, 32, 1)
        assert np.array_equal(w["U1"], r.model.get_weights()["U1"])


def test_cudnn_weight_conversion():
    """a file saved from CuDNNLSTM has bias [8W] and per-gate transposed kernels
    (Keras 2.3 saving semantics); loading converts back.
    NOT pinned by a reference artefact: no CuDNN-saved file exists offline, so the CuDNN-arranged input is built here from
    Keras' documented `convert_weights` rule (keras/engine/saving.py, `transform_kernels` with `from_cudnn=False`), written
    down independently of the function under test -- the test shows the two directions are inverse, not that either
    matches a real file."""
    rng = np.random.default_rng(0)
    W, D = 8, 12
    K, U, b = rng.standard_normal((D, 4 * W)), rng.standard_normal((W, 4 * W)), rng.standard_normal(4 * W)
    # forward direction of Keras' convert_weights(from_cudnn=False)
    Kc = np.hstack([g.T.reshape(g.shape, order='C') for g in np.hsplit(K, 4)])
    Uc = np.hstack([g.T for g in np.hsplit(U, 4)])
    bc = np.tile(0.5 * b, 2)
    K2, U2, b2 = modelio.convert_cudnn_lstm(Kc, Uc, bc, W)
    assert np.allclose(K2, K) and np.allclose(U2, U) and np.allclose(b2, b)
    K3, U3, b3 = modelio.convert_cudnn_lstm(K, U, b, W)          # plain files pass through
    assert K3 is K and U3 is U and b3 is b


def write_h5py_case(out):
    """the file test_h5py_reads_what_we_write pins, written by the h5lite writer (modelio without h5py) from seeded
    weights that need no LAPACK, so that its bytes are the same on every machine"""
    rng = np.random.default_rng(3)
    w = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in expected_weights().items()}
    config = {"history": json.dumps({"loss": [1.5]}), "width": 32, "depth": 2, "length": 16, "stateful": True,
              "variable_length": False, "mapping": np.arange(38, dtype=np.uint32)}
    h5py = modelio._h5py
    modelio._h5py = lambda: None
    try:
        modelio.save_model(out, w, config, 2, 1)
    finally:
        modelio._h5py = h5py
    return w


def test_h5py_reads_what_we_write():
    """h5py's reading of the file we write is recorded in tests/golden/h5py_readback.json (make_h5py_readback.py, h5py
    3.3) with the sha256 of that file: the file written here must be the one h5py read."""
    rec = json.load(open(os.path.join(GOLD, "h5py_readback.json")))
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "m.h5")
        w = write_h5py_case(out)
        with open(out, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == rec["sha256"], \
                "the writer's bytes changed: check them with h5py (tests/golden/make_h5py_readback.py)"
    assert rec["width"] == 32 and rec["width_shape"] == [] and rec["stateful"] is True
    assert rec["history"]["loss"] == [1.5]
    assert rec["mapping_dtype"] == "uint32" and rec["mapping_shape"] == [38]
    assert rec["layer_names"][2] == "char_embedding"
    assert rec["lstm_1_kernel"] == "lstm_1/kernel:0"
    assert abs(rec["lstm_1_kernel_3_5"] - float(w["K0"][3, 5])) < 1e-7
