"""Writes tests/golden/dgr_inlier_state_dict_keys.json: the state_dict keys and shapes of the reference's inlier network
ResUNetBN2C (GMF_DeepGlobalRegistration_{fpfh,fcgf}/model/resunet_new.py:424-721) for D = 6, in_channels = out_channels = 1,
both the fpfh variant (pe=False) and the fcgf variant (pe=True).

MinkowskiEngine is not needed: a minimal stand-in provides the module classes the network builds, with MinkowskiEngine
v0.5's parameter names and shapes as gmf_amd/sparse.py assumes them (`kernel` [k^D, Cin, Cout], or [Cin, Cout] when k^D = 1;
`bias` [1, Cout]; MinkowskiBatchNorm holding `bn`, a BatchNorm1d).  torchvision's weight download helper is stubbed too.  Run
on a machine that has the reference checkout; the tests read only the JSON.

Usage: python tests/tools/make_dgr_inlier_keys.py REFERENCE_ROOT"""
import argparse
import enum
import importlib
import json
import os
import sys
import types

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def install_stubs():
    ME = types.ModuleType("MinkowskiEngine")

    class RegionType(enum.Enum):
        HYPER_CUBE = 0
        HYPERCUBE = 0
        HYPER_CROSS = 1
        HYPERCROSS = 1

    class MinkowskiNetwork(nn.Module):
        def __init__(self, D):
            super().__init__()
            self.D = D

    class KernelGenerator:
        def __init__(self, kernel_size=-1, stride=1, dilation=1, is_transpose=False, region_type=0, dimension=-1, **kw):
            self.kernel_size, self.dimension = kernel_size, dimension

    class MinkowskiConvolution(nn.Module):
        def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False, kernel_generator=None,
                     dimension=None, **kw):
            super().__init__()
            K = kernel_size ** dimension
            self.kernel = nn.Parameter(torch.zeros((K, in_channels, out_channels) if K > 1 else (in_channels, out_channels)))
            self.bias = nn.Parameter(torch.zeros(1, out_channels)) if bias else None

    class MinkowskiConvolutionTranspose(MinkowskiConvolution):
        pass

    class MinkowskiBatchNorm(nn.Module):
        def __init__(self, num_features, eps=1e-5, momentum=0.1, **kw):
            super().__init__()
            self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum)

    ME.RegionType = RegionType
    ME.MinkowskiNetwork = MinkowskiNetwork
    ME.KernelGenerator = KernelGenerator
    ME.MinkowskiConvolution = MinkowskiConvolution
    ME.MinkowskiConvolutionTranspose = MinkowskiConvolutionTranspose
    ME.MinkowskiBatchNorm = MinkowskiBatchNorm
    ME.MinkowskiInstanceNorm = MinkowskiBatchNorm
    ME.MinkowskiReLU = nn.ReLU
    ME.MinkowskiELU = nn.ELU
    ME.SparseTensor = object
    MEF = types.ModuleType("MinkowskiEngine.MinkowskiFunctional")
    ME.MinkowskiFunctional = MEF
    sys.modules["MinkowskiEngine"] = ME
    sys.modules["MinkowskiEngine.MinkowskiFunctional"] = MEF
    tv = types.ModuleType("torchvision")
    tvm = types.ModuleType("torchvision.models")
    tvu = types.ModuleType("torchvision.models.utils")
    tvu.load_state_dict_from_url = lambda *a, **k: None
    tv.models, tvm.utils = tvm, tvu
    sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "torchvision.models.utils": tvu})
    for name in ("einops", "einops.layers", "einops.layers.torch"):
        try:
            importlib.import_module(name)
        except ImportError:
            pass


def keys_of(variant_dir):
    for m in [m for m in sys.modules if m == "model" or m.startswith("model.")]:
        del sys.modules[m]
    sys.path.insert(0, variant_dir)
    try:
        resnet = importlib.import_module("model.resnet")
        resnet.load_state_dict_from_url = lambda *a, **k: None
        orig = resnet.resnet34

        def no_download(*a, **k):
            k["pretrained"] = False
            return orig(*a, **k)
        resnet.resnet34 = no_download
        net = importlib.import_module("model.resunet_new").ResUNetBN2C(1, 1, D=6)
        return {k: list(v.shape) for k, v in net.state_dict().items()}
    finally:
        sys.path.remove(variant_dir)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference_root")
    args = ap.parse_args()
    install_stubs()
    dgr = os.path.join(args.reference_root, "GMF_DeepGlobalRegistration")
    out = {"pe=False": keys_of(os.path.join(dgr, "GMF_DeepGlobalRegistration_fpfh")),
           "pe=True": keys_of(os.path.join(dgr, "GMF_DeepGlobalRegistration_fcgf"))}
    path = os.path.join(ROOT, "tests", "golden", "dgr_inlier_state_dict_keys.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print(path, {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
