"""Generates tests/golden/reference_dataloading.pt from the REFERENCE'S OWN DataLoader3D.generate_train_batch
(3D/d_lka_former/training/dataloading/dataset_loading.py:155-379), GenericPreprocessor._run_internal
(3D/d_lka_former/preprocessing/preprocessing.py:318-354) and get_patch_size (training/data_augmentation/default_data_augmentation.py:107-127),
loaded from their files.

The loader runs after ``np.random.seed(s)`` on .npy files in a temporary folder.  batchgenerators is not installed: ``SlimDataLoaderBase`` is
stubbed by the three lines of its constructor the loader relies on, the file helpers by os.path's, and ``rotate_coords_3d / 2d`` are bound to
the restatement in deformablelka_amd.dataloading (batchgenerators 0.21's text).  generate_train_batch does not return its boxes: they are read
from its frame's local variables (bbox_x_lb ..., force_fg, selected_class, selected_voxel) by a sys.settrace hook while the function itself
runs unmodified.

_run_internal is driven through a temporary folder (a cropped .npz / .pkl in, the stage's .npz / .pkl out) with unit spacing, so that its
resampling is the identity, one 'nonCT' modality without the mask and the stubs of tests/golden/make_golden_preprocessing.py; its
num_samples = 10000 and 1 % are fixed in its text, so the rows recorded under "default" come from it.  The rows under "small"
(num_samples = 50, which reaches the 1 % branch at 7000 cells) come from lines 333-348 restated line by line in tests/dataloading_ref.py,
which this script first holds to _run_internal's result on every case.

The inputs are rebuilt by tests/dataloading_cases.py and only their SHA-256 is stored; expected batches and row sets are stored as SHA-256
too (the restatement tells which cell differs), boxes and draws as plain lists.
Run: python tests/golden/make_golden_dataloading.py"""
import contextlib
import importlib.util
import io
import os
import pickle
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import dataloading_cases as C     # noqa: E402
from tests import dataloading_ref as R       # noqa: E402
from deformablelka_amd import dataloading as D   # noqa: E402  (rotate_coords_*: host only)

REF = "/root/reference"
PKG = os.path.join(REF, "3D", "d_lka_former")


def from_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    mgp = from_file("make_golden_preprocessing", os.path.join(HERE, "make_golden_preprocessing.py"))
    _, pre = mgp.load_reference()
    pre.os, pre.pickle = os, pickle              # (what `from batchgenerators.utilities.file_and_folder_operations import *` brings)

    class SlimDataLoaderBase(object):
        def __init__(self, data, batch_size, number_of_threads_in_multithreaded=None):
            self._data = data
            self.batch_size = batch_size
            self.thread_id = 0

    def load_pickle(file, mode='rb'):
        with open(file, mode) as f:
            return pickle.load(f)

    files = sys.modules["batchgenerators.utilities.file_and_folder_operations"]
    files.__dict__.update(os=os, isfile=os.path.isfile, join=os.path.join, load_pickle=load_pickle)
    utils = sys.modules["batchgenerators.augmentations.utils"]
    utils.__dict__.update(random_crop_2D_image_batched=None, pad_nd_image=None, rotate_coords_3d=D.rotate_coords_3d,
                          rotate_coords_2d=D.rotate_coords_2d)
    m = types.ModuleType("batchgenerators.dataloading")
    m.SlimDataLoaderBase = SlimDataLoaderBase
    sys.modules["batchgenerators.dataloading"] = m
    m = types.ModuleType("d_lka_former.paths")
    m.preprocessing_output_dir = None
    sys.modules["d_lka_former.paths"] = m
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loading = from_file("d_lka_former_dataset_loading", os.path.join(PKG, "training", "dataloading", "dataset_loading.py"))
    return pre, loading


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def traced_batch(loader):
    """generate_train_batch() and, per sample, the locals it ended the sample's round with."""
    code = type(loader).generate_train_batch.__code__
    rows = {}

    def local(frame, event, arg):
        f = frame.f_locals
        try:                                     # (locals outlive a round: a row is complete, and last written, on the round's final lines)
            voxel = f.get("voxels_of_that_class") is not None if f["force_fg"] else False
            rows[int(f["j"])] = {"bbox_lb": [int(f["bbox_x_lb"]), int(f["bbox_y_lb"]), int(f["bbox_z_lb"])], "force_fg": bool(f["force_fg"]),
                                 "selected_class": int(f["selected_class"]) if voxel else -1,
                                 "selected_voxel": [int(v) for v in f["selected_voxel"]] if voxel else [-1, -1, -1]}
        except KeyError:
            pass
        return local

    def hook(frame, event, arg):
        return local if frame.f_code is code else None

    sys.settrace(hook)
    try:
        batch = loader.generate_train_batch()
    finally:
        sys.settrace(None)
    return batch, [rows[j] for j in range(loader.batch_size)]


def record_loader(loading, cid):
    data, (patch, final, B, p, mode, kwargs, seed, batches) = C.loader_inputs(cid)
    rec = {"inputs": C.inputs_digest(data), "batches": []}
    with tempfile.TemporaryDirectory() as tmp:
        dataset = {}
        for k, v in data.items():
            assert v["data"][0].size <= 20000
            np.save(os.path.join(tmp, k + ".npy"), v["data"])
            dataset[k] = {"data_file": os.path.join(tmp, k + ".npz"), "properties": v["properties"]}
        loader = loading.DataLoader3D(dataset, patch, final, B, False, p, "r", mode, kwargs)
        cases = {k: (v["data"].shape[1:], v["properties"]) for k, v in data.items()}
        rs, need = np.random.RandomState(seed), (np.array(patch) - np.array(final)).astype(int)
        np.random.seed(seed)
        for n in range(batches):
            batch, rows = quiet(traced_batch, loader)
            keys, boxes = R.draw_boxes(rs, cases, patch, need, B, p)                  # the restatement is held to what was recorded
            assert [str(k) for k in keys] == [str(k) for k in batch["keys"]] and boxes.tolist() == [r["bbox_lb"] for r in rows], (cid, n)
            rd, rseg = R.crop_batch([data[k]["data"] for k in keys], boxes, patch, mode, kwargs)
            assert batch["data"].dtype == np.float32 and C.same_bits(batch["data"], rd) and C.same_bits(batch["seg"], rseg), (cid, n)
            assert need.tolist() == loader.need_to_pad.tolist()
            rec["batches"].append({"keys": [str(k) for k in batch["keys"]], "bbox_lb": [r["bbox_lb"] for r in rows],
                                   "force_fg": [r["force_fg"] for r in rows], "selected_class": [r["selected_class"] for r in rows],
                                   "selected_voxel": [r["selected_voxel"] for r in rows], "need_to_pad": loader.need_to_pad.tolist(),
                                   "data": C.digest(batch["data"]), "seg": C.digest(batch["seg"])})
    return rec


def record_class_locations(pre, name):
    seg, classes = C.CL_CASES[name]()
    assert seg.size <= 20000 and float(seg.min()) >= -1.0
    data = ((C.noise((1,) + seg.shape, 90) - 0.5) * 10.0).astype(np.float32)
    g = pre.GenericPreprocessor({0: "nonCT"}, {0: False}, [0, 1, 2], None)
    with tempfile.TemporaryDirectory() as tmp:
        cropped, stage = os.path.join(tmp, "cropped"), os.path.join(tmp, "stage0")
        os.makedirs(cropped), os.makedirs(stage)
        np.savez_compressed(os.path.join(cropped, "case.npz"), data=np.vstack((data, seg[None])))
        with open(os.path.join(cropped, "case.pkl"), "wb") as f:
            pickle.dump({"original_spacing": np.array([1.0, 1.0, 1.0])}, f)
        quiet(g._run_internal, np.array([1.0, 1.0, 1.0]), "case", stage, cropped, None, classes)
        with open(os.path.join(stage, "case.pkl"), "rb") as f:
            props = pickle.load(f)
        stored = np.load(os.path.join(stage, "case.npz"))["data"]
    assert np.array_equal(stored[-1], seg), "the label map went through _run_internal unchanged (unit spacing)"
    own = props["class_locations"]
    restated = R.class_locations(seg, classes)
    assert list(own.keys()) == classes
    for c in classes:
        assert np.array_equal(np.asarray(own[c]), np.asarray(restated[c])), (name, c)
    return {"input": C.digest(seg), "default": C.locations_digest(own), "small": C.locations_digest(R.class_locations(seg, classes, **C.CL_SMALL))}


def record_patch_sizes():
    # default_data_augmentation.py imports the whole transform zoo; the function stands alone: evaluate lines 107-127
    with open(os.path.join(PKG, "training", "data_augmentation", "default_data_augmentation.py")) as f:
        src = f.read()
    body = src[src.index("def get_patch_size("):]
    body = body[:body.index("\ndef get_default_augmentation(")]
    ns = {"np": np}
    exec(compile(body, "default_data_augmentation.py:107-127", "exec"), ns)
    aug = types.SimpleNamespace(get_patch_size=ns["get_patch_size"])
    r30, r15, r180 = 30. / 360 * 2. * np.pi, 15. / 360 * 2. * np.pi, np.pi
    calls = [((64, 128, 128), (-r30, r30), (-r30, r30), (-r30, r30), (0.85, 1.25)),        # the Synapse trainer's (:397-427)
             ((64, 128, 128), (-r30, r30), (-r30, r30), (-r30, r30), (0.7, 1.4)),
             ((8, 12, 10), (-r30, r30), (-r30, r30), (-r30, r30), (0.7, 1.4)),
             ((16, 160, 160), (-r180, r180), (0, 0), (0, 0), (0.85, 1.25)),
             ((160, 160), (-r180, r180), (0, 0), (0, 0), (0.85, 1.25)),                      # two extents: rotate_coords_2d
             ((96, 96, 96), r15, r15, r15, (0.85, 1.25))]
    return [(args, [int(v) for v in aug.get_patch_size(*args)]) for args in calls]


def main():
    pre, loading = load_reference()
    out = {"numpy": np.__version__, "loader": {}, "class_locations": {}}
    for cid in C.LOADER_CALLS:
        out["loader"][cid] = record_loader(loading, cid)
    a, c = out["loader"]["aliasing"]["batches"], out["loader"]["constant2"]["batches"]
    assert a[0]["keys"][0] == "small" and a[0]["need_to_pad"] == [1, 3, 0] == a[-1]["need_to_pad"] and len(a) == 3
    assert all(b["force_fg"] == [False, False, True] for b in a + c)                          # round(3 * 0.67) = 2
    forced = [(b["keys"][2], b["selected_class"][2], b["bbox_lb"][2]) for b in c]
    assert any(k == "nofg" and cls == -1 for k, cls, _ in forced), forced                      # no foreground: random boxes
    assert any(k == "corner" and cls == 2 and all(lb[d] + C.PATCH[d] > e for d, e in enumerate((11, 13, 17))) for k, cls, lb in forced), forced
    for name in C.CL_CASES:
        out["class_locations"][name] = record_class_locations(pre, name)
    out["patch_size"] = record_patch_sizes()
    assert out["patch_size"][0][1] == D.get_patch_size(*out["patch_size"][0][0]).tolist()
    path = os.path.join(HERE, "reference_dataloading.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")
    for cid, rec in out["loader"].items():
        for n, b in enumerate(rec["batches"]):
            print(cid, n, b["keys"], b["bbox_lb"], b["selected_class"], b["need_to_pad"])
    for name, rec in out["class_locations"].items():
        print(name, {c: v[0] for c, v in rec["default"].items()}, {c: v[0] for c, v in rec["small"].items()})
    for args, want in out["patch_size"]:
        print("patch size", args[0], "->", want)


if __name__ == "__main__":
    main()
