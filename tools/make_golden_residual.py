"""Capture tests/golden/vnet_la_residual_tiny.npz from the REFERENCE's residual V-Net, networks/VNet.py VNet(has_residual=True)
(ResidualConvBlock, networks/VNet.py:35-65):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_residual.py --reference <checkout of the reference>/code

The reference is imported at run time only (nothing of its source travels: the fixture holds seeds, inputs and results).  One forward and
backward in fp64 on the CPU at 2 x 1 x 32 x 32 x 16, train mode, parameters from oracle/bcp_oracle.py init_params(seed = PARAM_SEED,
random_affine = True) -- the seed is stored, not the parameters.  The net is called as decoder(encoder(x)): the reference's MaxPool3d on
the deepest level raises at this size and feeds only the dead second return value.  Its two nn.Dropout3d modules are replaced by a
stand-in that multiplies with an injected keep mask (x 2), the masks are stored.  The loss is the oracle's sup_loss_la of the
reference's logits.  No test calls this script; tests/residual_checks.py reads the fixture.

Keys: x, tgt, drop_x5, drop_x9, param_seed, logits, loss, grad_names, grad_norms (L2 norm per parameter gradient, in named_parameters()
order), six gradient tensors (grad_*), rm_* / rv_* of block_one and block_nine after the pass, n_keys (len(state_dict()))."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_SEED = 211
DATA_SEED = 212
SHAPE = (32, 32, 16)
NAMED = (("grad_block_one_w", "encoder.block_one.conv.0.weight"), ("grad_block_nine_w", "decoder.block_nine.conv.0.weight"),
         ("grad_eight_up_w", "decoder.block_eight_up.conv.0.weight"), ("grad_one_dw_w", "encoder.block_one_dw.conv.0.weight"),
         ("grad_out_conv_w", "decoder.out_conv.weight"), ("grad_bn1_w", "encoder.block_one.conv.1.weight"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's code/ directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vnet_la_residual_tiny.npz"))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    import torch
    import torch.nn as nn
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import bcp_oracle as O
    sys.path.insert(0, os.path.abspath(args.reference))
    from networks.VNet import VNet as RefVNet

    class InjectedDrop(nn.Module):
        """nn.Dropout3d(p=0.5) with a given keep mask [N, C]"""
        mask = None

        def forward(self, x):
            return x if self.mask is None else x * self.mask.view(x.shape[0], -1, 1, 1, 1).to(x.dtype) * 2.0

    P = O.init_params(O.vnet_param_shapes(), seed=PARAM_SEED, random_affine=True)
    net = RefVNet(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True, has_residual=True)
    plain = RefVNet(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True, has_residual=False)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(v.shape)) for k, v in plain.state_dict().items()]
    assert [n for n, _ in net.named_parameters()] == [n for n, _ in plain.named_parameters()]
    net.load_state_dict(P, strict=True)
    net.double().train()
    rng = np.random.default_rng(DATA_SEED)
    x = torch.from_numpy(rng.standard_normal((2, 1) + SHAPE, dtype=np.float32))
    tgt = torch.from_numpy(rng.integers(0, 2, (2,) + SHAPE))
    dm = {"x5": torch.from_numpy((rng.random((2, 256)) < 0.5).astype(np.float32)), "x9": torch.from_numpy((rng.random((2, 16)) < 0.5).astype(np.float32))}
    net.encoder.dropout, net.decoder.dropout = InjectedDrop(), InjectedDrop()
    net.encoder.dropout.mask, net.decoder.dropout.mask = dm["x5"], dm["x9"]
    out, _ = net.decoder(net.encoder(x.double()))
    loss = O.sup_loss_la(out, tgt)
    loss.backward()
    grads = [(n, p.grad) for n, p in net.named_parameters() if p.grad is not None]
    g = dict(grads)
    sd = net.state_dict()
    np.savez_compressed(
        args.out, x=x.numpy(), tgt=tgt.numpy().astype(np.uint8), drop_x5=dm["x5"].numpy().astype(np.uint8), drop_x9=dm["x9"].numpy().astype(np.uint8),
        param_seed=np.int64(PARAM_SEED), logits=out.detach().numpy(), loss=np.float64(loss.item()),
        grad_names=np.array([n for n, _ in grads]), grad_norms=np.array([float(v.norm()) for _, v in grads]),
        rm_block_one=sd["encoder.block_one.conv.1.running_mean"].numpy(), rv_block_one=sd["encoder.block_one.conv.1.running_var"].numpy(),
        rm_block_nine=sd["decoder.block_nine.conv.1.running_mean"].numpy(), rv_block_nine=sd["decoder.block_nine.conv.1.running_var"].numpy(),
        n_keys=np.int64(len(sd)), **{key: g[name].numpy() for key, name in NAMED})
    print("wrote", args.out, os.path.getsize(args.out), "bytes;", len(grads), "gradients, loss", float(loss.detach()))


if __name__ == "__main__":
    main()
