"""test_LA for checkpoints of a V-Net with another normalisation: the command line and the flow of bcp_amd/test_LA.py (the reference's
code/test_LA.py:9-52 plus this build's flags), plus `--normalization {batchnorm,groupnorm}` -- the norm layers the checkpoint was trained
with (`LA_BCP_train --normalization`, networks/VNet.py:20-21) -- and `--has_residual` for checkpoints of a residual V-Net
(`LA_BCP_train --has_residual`, networks/VNet.py:35-65).  A residual checkpoint has the plain net's keys: reading it without the flag (or
a plain one with it) loads, and evaluates another function; the flag is logged.

Why a module of its own: bcp_amd/test_LA.py carries a `test_*.py` name, and a feature change leaves every existing `test_*.py` file
byte-identical, so the option cannot be added there.  This module takes test_LA's parser as its parent and runs
test_LA's own `test_calculate_metric` with the factory bound to the chosen normalisation; nothing else differs.  A checkpoint of the other
normalisation fails in `load_state_dict`.

  python -m bcp_amd.eval_LA --labelnum 8 --stage_name self_train --normalization groupnorm
"""
import argparse
import functools
import logging
import sys

from bcp_amd import test_LA as _T
from bcp_amd.networks.net_factory import net_factory

parser = argparse.ArgumentParser(parents=[_T.parser], conflict_handler="resolve")
parser.add_argument("--normalization", type=str, default="batchnorm", choices=("batchnorm", "groupnorm"),
                    help="the norm layers the checkpoint was trained with (LA_BCP_train --normalization); a checkpoint of the other kind fails to load")
parser.add_argument("--has_residual", action="store_true",
                    help="the checkpoint is a residual V-Net's (LA_BCP_train --has_residual); the keys are the plain net's, so a mismatch cannot fail on load")


def main(argv=None):
    FLAGS = parser.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s.%(msecs)03d] %(message)s", datefmt="%H:%M:%S", stream=sys.stdout)
    factory = _T.net_factory
    _T.net_factory = functools.partial(net_factory, normalization=FLAGS.normalization, has_residual=FLAGS.has_residual)
    logging.info("V-Net: normalization %s, %s blocks", FLAGS.normalization, "residual" if FLAGS.has_residual else "plain")
    try:
        return _T.test_calculate_metric(FLAGS)
    finally:
        _T.net_factory = factory


if __name__ == "__main__":
    print(main())
