"""The offline LA evaluation of this build: the reference's command line (code/test_LA.py:9-17 -- every flag with its default) and its
flow (:19-52 with utils/test_3d_patch.py:40-80): <model>_best_model.pth of a training stage -> sliding-window inference of every case of
the test list -> largest component (--nms) -> Dice, Jaccard, 95HD, ASD per case and averaged -> performance.txt.

Everything heavy runs on the device through functions the training side already uses: the eval-mode V-Net, the sliding-window
accumulation, the largest component, the overlap counts and the surface distances (utils/test_3d_patch.py, utils/surface.py -- the loop
is surface.la_all_case, the one validation uses).  Cases come from <root_path>/test.list through dataloaders/h5_datasets.LAHeart and
its device cache; without that list file, synthetic cases stand in, as in LA_BCP_train.

Differences from the reference, on purpose: --stage_name pre_train works (its {'net','opt'} checkpoint is read too, utils/evaluate.py);
--gpu is accepted and not applied (the current device is used, as in the drivers); --save_result writes .npy files, not nifti.

  python -m bcp_amd.test_LA --labelnum 8 --stage_name self_train
"""
import argparse
import logging
import os
import sys

from bcp_amd.networks.net_factory import net_factory
from bcp_amd.utils import evaluate, surface

# (flag, type, default) -- the reference's CLI, then this build's additions
_REFERENCE_FLAGS = (
    ("root_path", str, "/data/byh_data/SSNet_data/LA/"), ("exp", str, "BCP"), ("model", str, "VNet"), ("gpu", str, "0"),
    ("detail", int, 1), ("nms", int, 1), ("labelnum", int, 4), ("stage_name", str, "self_train"),
)
_BUILD_FLAGS = (
    ("cases", int, 2, "synthetic test volumes when <root_path>/test.list does not exist"),
)
parser = argparse.ArgumentParser()
for _name, _type, _default in _REFERENCE_FLAGS:
    parser.add_argument("--" + _name, type=_type, default=_default)
for _name, _type, _default, _help in _BUILD_FLAGS:
    parser.add_argument("--" + _name, type=_type, default=_default, help=_help)
parser.add_argument("--patch_size", type=int, nargs=3, default=[112, 112, 80], help="sliding-window patch (test_LA.py:43)")
parser.add_argument("--stride", type=int, nargs=2, default=[18, 4], help="sliding-window strides (xy, z) (test_LA.py:43)")
parser.add_argument("--save_result", action="store_true", help="write %%02d_pred.npy / _img.npy / _gt.npy per case into the predictions directory")
parser.add_argument("--no_surface", action="store_true", help="report hd95 / asd as nan and launch none of the surface-distance kernels")

num_classes = 2


def _cases(FLAGS, device):
    """the test list's cases as (image, label) device tensors, or the synthetic stand-ins"""
    if os.path.exists(os.path.join(FLAGS.root_path, "test.list")):
        from bcp_amd.dataloaders.h5_datasets import LAHeart
        db = LAHeart(base_dir=FLAGS.root_path, split="test", device=device)
        return [(s["image"], s["label"]) for s in (db[i] for i in range(len(db)))]
    logging.info("no {}/test.list: synthetic LA-like cases".format(FLAGS.root_path))
    return evaluate.synthetic_la_cases(FLAGS.cases, FLAGS.patch_size, device)


def test_calculate_metric(FLAGS):
    """:34-47 -> the averaged [dice, jc, hd95, asd]"""
    snapshot_path = "./model/BCP/LA_{}_{}_labeled/{}".format(FLAGS.exp, FLAGS.labelnum, FLAGS.stage_name)
    test_save_path = "./model/BCP/LA_{}_{}_labeled/{}_predictions/".format(FLAGS.exp, FLAGS.labelnum, FLAGS.model)
    os.makedirs(test_save_path, exist_ok=True)
    print(test_save_path)
    model = net_factory(net_type=FLAGS.model, in_chns=1, class_num=num_classes, mode="test")
    save_model_path = os.path.join(snapshot_path, "{}_best_model.pth".format(FLAGS.model))
    evaluate.load_weights(model, save_model_path)
    print("init weight from {}".format(save_model_path))
    model.eval()
    cases = _cases(FLAGS, next(model.parameters()).device)

    def on_case(ith, image, label, prediction, single_metric):
        if FLAGS.detail:                                             # utils/test_3d_patch.py:62-63
            print("%02d,\t%.5f, %.5f, %.5f, %.5f" % ((ith,) + tuple(single_metric)))
        if FLAGS.save_result:
            evaluate.save_case(test_save_path, "%02d" % ith, prediction, image, label)

    avg_metric = surface.la_all_case(model, cases, num_classes=num_classes, patch_size=tuple(FLAGS.patch_size), stride_xy=FLAGS.stride[0],
                                     stride_z=FLAGS.stride[1], nms=FLAGS.nms, surface=not FLAGS.no_surface, on_case=on_case)
    print("average metric is {}".format(avg_metric))
    evaluate.write_performance(test_save_path, ["average metric is {} ".format(avg_metric)])
    return avg_metric


test_calculate_metric.__test__ = False   # name mirrors the reference module; not a pytest test


def main(argv=None):
    FLAGS = parser.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s.%(msecs)03d] %(message)s", datefmt="%H:%M:%S", stream=sys.stdout)
    return test_calculate_metric(FLAGS)


if __name__ == "__main__":
    print(main())
