"""Capture tests/golden/mask_strategies.npz from the REFERENCE's four non-default masking functions:

    utils/BCP_utils.py   random_mask (:30), concate_mask (:48)          3-D, shapes (112,112,80) and (96,96,96)
    ACDC_BCP_train.py    random_mask (:142), contact_mask (:156)        2-D, shape (256,256)

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_masks.py --reference <checkout of the reference>/code

The reference is imported at run time only (nothing of its source travels: the fixture holds seeds and results).  It is run on the CPU: the
modules it imports but this capture never calls are replaced by empty stand-ins when they are absent, and its unconditional .cuda() calls
return the tensor itself.  No test calls this script; tests/mask_checks.py reads the fixture.

Per case `<name>` the file holds: `<name>/seed`; `<name>/shape` (the spatial shape); `<name>/bits` = np.packbits of the dense image mask
(1 = keep, 0 = pasted region); `<name>/batch` = the loss mask's batch size (every sample of the loss mask is checked to equal the image mask
before it is dropped); `<name>/next` = np.random.randint(0, 1 << 30) drawn right after the call, which pins how many draws the call made.
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 2, 1337, 2020)
BATCH = 2


class _Anything:
    """stand-in object: callable, subscriptable by attribute, never used by the four functions captured here"""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Anything()

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything()


def _stand_in(name):
    mod = types.ModuleType(name)
    mod.__file__ = "<stand-in %s>" % name
    mod.__path__ = []
    mod.__getattr__ = lambda attr: (_ for _ in ()).throw(AttributeError(attr)) if attr.startswith("__") else _Anything
    sys.modules[name] = mod
    parent, _, leaf = name.rpartition(".")
    if parent:
        if parent not in sys.modules:
            _stand_in(parent)
        setattr(sys.modules[parent], leaf, mod)
    return mod


def _import_with_stand_ins(name, tries=64):
    """import `name`; every third-party module that is not installed here becomes a stand-in and the import is tried again"""
    for _ in range(tries):
        try:
            return importlib.import_module(name)
        except ModuleNotFoundError as e:
            if not e.name or e.name == name:
                raise
            _stand_in(e.name)
            sys.modules.pop(name, None)
    raise RuntimeError("could not import %s" % name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's code/ directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mask_strategies.npz"))
    args = ap.parse_args()
    sys.dont_write_bytecode = True

    import torch
    import torch.nn as nn
    torch.Tensor.cuda = lambda self, *a, **k: self      # no GPU in the capture: .cuda() is unconditional in the reference
    nn.Module.cuda = lambda self, *a, **k: self

    sys.path.insert(0, os.path.abspath(args.reference))
    sys.argv = [sys.argv[0]]                            # the reference's scripts parse the command line on import
    ref_utils = _import_with_stand_ins("utils.BCP_utils")
    ref_acdc = _import_with_stand_ins("ACDC_BCP_train")

    cases = []
    for shape in ((112, 112, 80), (96, 96, 96)):
        tag = "x".join(str(v) for v in shape)
        cases += [("random3d_" + tag, ref_utils.random_mask, shape), ("concat3d_" + tag, ref_utils.concate_mask, shape)]
    cases += [("random2d_256x256", ref_acdc.random_mask, (256, 256)), ("contact2d_256x256", ref_acdc.contact_mask, (256, 256))]

    out = {}
    for name, fn, shape in cases:
        img = torch.zeros((BATCH, 1) + shape)
        for seed in SEEDS:
            np.random.seed(seed)
            mask, loss_mask = fn(img)
            nxt = int(np.random.randint(0, 1 << 30))
            m = mask.numpy()
            assert m.shape == shape and set(np.unique(m)) <= {0, 1}
            lm = loss_mask.numpy()
            assert lm.shape == (BATCH,) + shape and all((lm[i] == m).all() for i in range(BATCH))
            key = "%s/s%d" % (name, seed)
            out[key + "/seed"] = np.int64(seed)
            out[key + "/shape"] = np.asarray(shape, dtype=np.int64)
            out[key + "/bits"] = np.packbits(m.astype(np.uint8).reshape(-1))
            out[key + "/batch"] = np.int64(lm.shape[0])
            out[key + "/next"] = np.int64(nxt)
            print("%-32s zero fraction %.4f  next draw %d" % (key, 1.0 - m.mean(), nxt))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
