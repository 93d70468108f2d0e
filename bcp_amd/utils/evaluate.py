"""What the offline evaluation entry points share (bcp_amd/test_LA.py, bcp_amd/test_ACDC.py, pancreas/train_pancreas.py test_model):
reading a checkpoint, the synthetic stand-in cases, `performance.txt` and the saved predictions.

  load_weights(net, path)                     a bare state_dict (what self-training writes) or {'net': ...} with or without 'opt' / 'epoch'
                                              (what pre-training and the pancreas driver write).  The reference's test_LA.py:37 reads only the
                                              first, so its --stage_name pre_train cannot work; here both do.  A missing file raises
                                              FileNotFoundError naming the path.
  synthetic_la_cases(n, patch_size, device)   [(image, label)] -- the volumes LA_BCP_train._val_cases makes, sized from `patch_size`
  synthetic_acdc_volumes(n, patch_size, dev)  [(case, image [S,X,Y], label [S,X,Y])] -- the volumes ACDC_BCP_train._val_set makes
  write_performance(test_save_path, lines)    <test_save_path>/../performance.txt, where the reference writes it
                                              (utils/test_3d_patch.py:77-78, test_ACDC.py:115-117)
  save_case(test_save_path, stem, prediction, image, label)   <stem>_pred.npy, <stem>_img.npy, <stem>_gt.npy (float32, as the reference casts)

Saved predictions are .npy files: the reference writes nifti through nibabel (test_3d_patch.py:68-71) or SimpleITK (test_ACDC.py:70-78,
commented out there); neither library is installed where this repository is built, so nifti output is out of scope.
"""
import os

import numpy as np
import torch

_SYNTH_SEED = 1337      # the drivers' --seed default: a default evaluation walks the volumes a default training run validated on


def load_weights(net, path):
    path = str(path)
    if not os.path.isfile(path):
        raise FileNotFoundError("no checkpoint at {}".format(path))
    device = next(net.parameters()).device
    ckpt = torch.load(path, map_location=device)
    if isinstance(ckpt, dict) and "net" in ckpt and isinstance(ckpt["net"], dict):
        ckpt = ckpt["net"]
    from ..pancreas.pancreas_utils import _from_ref_keys      # the pancreas driver writes the reference's nn.DataParallel keys (save_net)
    net.load_state_dict(_from_ref_keys(ckpt))
    return net


def synthetic_la_cases(n, patch_size, device, seed=_SYNTH_SEED):
    """LA_BCP_train._val_cases: volumes a little larger than the patch, so the sliding window takes several positions per axis"""
    from .. import synth
    n = max(int(n), 1)
    shape = (patch_size[0] + 16, patch_size[1] + 8, patch_size[2] + 8)
    vols, labs = synth.la_batch(n, shape=shape, seed=seed + 99)
    return [(vols[i, 0].to(device), labs[i].to(device)) for i in range(n)]


def synthetic_acdc_volumes(n, patch_size, device, seed=_SYNTH_SEED):
    """ACDC_BCP_train._val_set: volumes of 8 slices at the training resolution, named synth_00, synth_01, ..."""
    from .. import synth
    out = []
    for i in range(max(int(n), 1)):
        vols, labs = synth.acdc_batch(8, shape=tuple(patch_size), seed=seed + 500 + i)
        out.append(("synth_%02d" % i, vols[:, 0].to(device), labs.to(device)))
    return out


def write_performance(test_save_path, lines):
    """-> the path written.  `lines` are written as they are, one per line."""
    target = os.path.join(os.path.dirname(os.path.normpath(test_save_path)), "performance.txt")
    with open(target, "w") as f:
        f.writelines(line + "\n" for line in lines)
    return target


def _f32(a):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float32)


def save_case(test_save_path, stem, prediction, image, label):
    for name, a in (("pred", prediction), ("img", image), ("gt", label)):
        np.save(os.path.join(test_save_path, "{}_{}.npy".format(stem, name)), _f32(a))
