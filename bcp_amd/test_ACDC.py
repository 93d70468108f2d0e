"""The offline ACDC evaluation of this build: the reference's command line (code/test_ACDC.py:17-23 -- every flag with its default) and
its flow (:36-117): <model>_best_model.pth of a training stage -> every volume of the test list through the eval-mode 2-D U-Net slice by
slice -> Dice, Jaccard, 95HD, ASD of the [S,X,Y] volume for each of the classes 1, 2, 3, averaged over the volumes -> performance.txt.

The label volume is built by utils/val_2d.predict_volume, the function validation uses (zoom to the patch size, eval net, first-max argmax,
zoom back, all on the device); the per-class metrics are utils/surface.acdc_case_metrics (integer overlap counts and the surface-distance
kernels).  Volumes are read from <root_path>/data/<case>.h5 through dataloaders/h5_datasets.read_h5; without <root_path>/test.list,
synthetic volumes stand in, as in ACDC_BCP_train.

Differences from the reference, on purpose:
  * the reference deletes an existing predictions directory (shutil.rmtree, :88-89).  Here the directory is created if needed and only the
    files this run writes are overwritten: an evaluation does not remove files it did not make.
  * --stage_name pre_train works (its {'net','opt'} checkpoint is read too, utils/evaluate.py).
  * --save_result writes <case>_pred.npy / _img.npy / _gt.npy; the reference's nifti output (SimpleITK, commented out at :76-78) is out
    of scope, the library is not installed where this repository is built.

  python -m bcp_amd.test_ACDC --labelnum 7 --stage_name self_train
"""
import argparse
import logging
import os
import sys

import numpy as np
import torch

from bcp_amd.networks.net_factory import net_factory
from bcp_amd.utils import evaluate, surface, val_2d

# (flag, type, default) -- the reference's CLI, then this build's additions
_REFERENCE_FLAGS = (
    ("root_path", str, "/data/byh_data/SSNet_data/ACDC"), ("exp", str, "BCP"), ("model", str, "unet"), ("num_classes", int, 4),
    ("labelnum", int, 3), ("stage_name", str, "self_train"),
)
_BUILD_FLAGS = (
    ("cases", int, 2, "synthetic test volumes when <root_path>/test.list does not exist"),
)
parser = argparse.ArgumentParser()
for _name, _type, _default in _REFERENCE_FLAGS:
    parser.add_argument("--" + _name, type=_type, default=_default)
for _name, _type, _default, _help in _BUILD_FLAGS:
    parser.add_argument("--" + _name, type=_type, default=_default, help=_help)
parser.add_argument("--patch_size", type=int, nargs=2, default=[256, 256], help="the resolution every slice is zoomed to (test_ACDC.py:44)")
parser.add_argument("--save_result", action="store_true", help="write <case>_pred.npy / _img.npy / _gt.npy into the predictions directory")
parser.add_argument("--no_surface", action="store_true", help="report hd95 / asd as nan and launch none of the surface-distance kernels")


def _volumes(FLAGS, device):
    """[(case, image [S,X,Y] float32, label [S,X,Y] uint8)] on the device: the sorted test list (:83-85), or the synthetic stand-ins"""
    list_path = os.path.join(FLAGS.root_path, "test.list")
    if not os.path.exists(list_path):
        logging.info("no {}/test.list: synthetic ACDC-like volumes".format(FLAGS.root_path))
        return evaluate.synthetic_acdc_volumes(FLAGS.cases, FLAGS.patch_size, device)
    from bcp_amd.dataloaders import h5_datasets
    with open(list_path, "r") as f:
        image_list = sorted(item.replace("\n", "").split(".")[0] for item in f.readlines() if item.strip())
    out = []
    for case in image_list:
        image, label = h5_datasets.read_h5(FLAGS.root_path + "/data/{}.h5".format(case))
        out.append((case, torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(device),
                    torch.from_numpy(np.ascontiguousarray(label).astype(np.uint8)).to(device)))
    return out


def test_single_volume(case, image, label, net, test_save_path, FLAGS):
    """:36-79 -> (first_metric, second_metric, third_metric), each (dice, jc, hd95, asd)"""
    device = next(net.parameters()).device
    image = image.to(device=device, dtype=torch.float32)
    label = label.to(device=device, dtype=torch.uint8).contiguous()
    prediction = val_2d.predict_volume(image, net, tuple(FLAGS.patch_size))
    metrics = surface.acdc_case_metrics(prediction, label, surface=not FLAGS.no_surface, classes=FLAGS.num_classes)
    if FLAGS.save_result:
        evaluate.save_case(test_save_path, case, prediction, image, label)
    return metrics


test_single_volume.__test__ = False   # name mirrors the reference module; not a pytest test


def Inference(FLAGS):
    """:82-107 -> (avg_metric: one array [dice, jc, hd95, asd] per class, test_save_path)"""
    snapshot_path = "./model/BCP/ACDC_{}_{}_labeled/{}".format(FLAGS.exp, FLAGS.labelnum, FLAGS.stage_name)
    test_save_path = "./model/BCP/ACDC_{}_{}_labeled/{}_predictions/".format(FLAGS.exp, FLAGS.labelnum, FLAGS.model)
    os.makedirs(test_save_path, exist_ok=True)
    net = net_factory(net_type=FLAGS.model, in_chns=1, class_num=FLAGS.num_classes)
    save_model_path = os.path.join(snapshot_path, "{}_best_model.pth".format(FLAGS.model))
    evaluate.load_weights(net, save_model_path)
    print("init weight from {}".format(save_model_path))
    net.eval()
    volumes = _volumes(FLAGS, next(net.parameters()).device)
    totals = [np.zeros(4) for _ in range(1, FLAGS.num_classes)]
    for case, image, label in volumes:
        for total, single in zip(totals, test_single_volume(case, image, label, net, test_save_path, FLAGS)):
            total += np.asarray(single, dtype=np.float64)
    avg_metric = [total / len(volumes) for total in totals]
    return avg_metric, test_save_path


def main(argv=None):
    FLAGS = parser.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s.%(msecs)03d] %(message)s", datefmt="%H:%M:%S", stream=sys.stdout)
    metric, test_save_path = Inference(FLAGS)
    print(metric)
    mean = sum(metric) / len(metric)
    print(mean)
    evaluate.write_performance(test_save_path, ["metric is {} ".format(metric), "average metric is {}".format(mean)])      # :115-117
    return metric, test_save_path


if __name__ == "__main__":
    main()
