"""Helpers of the image-encoder tests (gmf_amd/csrc/image_kernels.hip): float64 references, the dispatcher's rules recomputed
on the host, the weight images unpacked by the unit formulas of the kernels' header comments, and a CPU emulation of the
split-fp16 arithmetic.  Nothing here needs a GPU.

Tolerances
  conv / stem rule      err < max(4 floor, 4e-6), floor = torch's own float32 evaluation against the float64 reference;
  small-operand bound   err <= 4 floor + 2^-25 max_co sum |W[co]|   (`split_bound`): an activation x travels as hi = fp16(x) and
                        lo = fp16(x - hi).  x - hi is exact in fp32; lo rounds it to fp16, whose spacing never falls below the
                        subnormal quantum 2^-24.  For |x| < 2^-3 the residual |x - hi| <= 2^-12 |x| lies below the smallest normal
                        fp16 number 2^-14, so lo is off by at most half a quantum, 2^-25, whatever the scale of x, and an output
                        channel collects at most 2^-25 sum |W[co]| of it.  Nothing else in the split loses anything at these
                        scales (the hi x hi, hi x lo and lo x hi products are exact in fp32; the dropped lo x lo term is below
                        2^-24 |x w|), and the fp32 accumulation is what `floor` measures."""
import re
from collections import Counter

import torch
import torch.nn.functional as F

H2_SCALE = 256.0

# the eight shapes of the original convolution test and three more: W = 48 (the widest patch), a single pixel, W = 49 at 128 channels
CONV_SHAPES = [(64, 64, 3, 1, 30, 40), (64, 128, 3, 2, 30, 40), (128, 128, 3, 1, 15, 20), (64, 128, 1, 2, 30, 40),
               (64, 64, 3, 1, 7, 5), (64, 128, 3, 2, 9, 11), (128, 128, 3, 1, 5, 48), (64, 64, 3, 1, 3, 50),
               (64, 64, 3, 1, 2, 48), (64, 64, 3, 1, 1, 1), (128, 128, 3, 1, 4, 49)]


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


# ---- the dispatcher's rules (launch_conv_nhwc_h2, launch_stem_h2), recomputed ----------------------------------------------------
def conv_out_size(H, W, ks, stride):
    pad = ks // 2
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def conv_workgroups(B, H, W, cout, ks, stride):
    """Workgroups of the 128-pixel kernels: ceil(P / 128) x (cout / 64)."""
    Ho, Wo = conv_out_size(H, W, ks, stride)
    return ((B * Ho * Wo + 127) // 128) * (cout // 64)


def expected_conv_kernel(B, H, W, cin, cout, ks, stride, small_grid=1, lds_patch=1):
    """(kernel name, template arguments) launch_conv_nhwc_h2 chooses; bools as the demangler prints them."""
    nwg = conv_workgroups(B, H, W, cout, ks, stride)
    cbt = ks == 3 and stride == 1
    if nwg < 128 and small_grid:
        return "k_conv_small_h2", (cin, cout, ks, stride, cbt, 8 if cin == 128 else 4)
    if lds_patch and cbt and W <= 48 and cin == cout:
        if cin == 64 and W <= 40 and lds_patch == 1 and 512 < nwg <= 768:
            return "k_conv3x3_patch_h2", (64, 64, 3, 40, False, 3)
        return "k_conv3x3_patch_h2", (cin, cin, 4, 48, True, 2)
    return "k_conv_nhwc_h2", (cin, cout, ks, stride, cbt)


def stem_out_size(H, W):
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1


def stem_workgroups(B, H, W):
    """Workgroups of the 8 x 8 form."""
    Hp, Wp = stem_out_size(H, W)
    return ((Wp + 7) // 8) * ((Hp + 7) // 8) * B


def expected_stem_kernel(B, H, W, small_grid=1):
    return "k_stem_h2", (4 if stem_workgroups(B, H, W) < 128 and small_grid else 8,)


# ---- which kernels ran ------------------------------------------------------------------------------------------------------
_KERNEL = re.compile(r"gmf::(?:\(anonymous namespace\)::)?(k_\w+)\s*(?:<([^<>]*)>)?")


def _targ(s):
    s = s.strip()
    if s in ("true", "false"):
        return s == "true"
    m = re.fullmatch(r"\(?(?:bool|int)?\)?\s*(-?\d+)", s)
    return int(m.group(1)) if m else s


def parse_kernel(key):
    """Profiler key -> (name, template arguments or None when the key carries none), or None for a kernel outside gmf::."""
    m = _KERNEL.search(key)
    if not m:
        return None
    return m.group(1), (tuple(_targ(a) for a in m.group(2).split(",")) if m.group(2) is not None else None)


def launched(fn):
    """(fn(), Counter of the gmf:: kernels it launched as (name, template arguments)), from the torch profiler's device activities."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = Counter()
    for e in prof.key_averages():
        k = parse_kernel(e.key)
        if k and e.device_time_total > 0:
            names[k] += e.count
    return out, names


def assert_ran(names, expected, what="", count=1):
    """Exactly the expected kernel ran, `count` times, with the expected template arguments, and no other gmf:: kernel."""
    assert len(names) == 1 and sum(names.values()) == count, (what, dict(names), expected)
    (name, targs), = names.keys()
    assert name == expected[0] and targs is not None, (what, name, targs, expected)
    assert tuple(int(a) for a in targs) == tuple(int(a) for a in expected[1]), (what, name, targs, expected)


# ---- float64 references ---------------------------------------------------------------------------------------------------------
def conv_case(cin, cout, ks, stride, B, H, W, seed, scale=1.0):
    """Seeded inputs of one convolution case and its float64 / float32 results without residual or ReLU."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=gen) * scale
    Wt = torch.randn(cout, cin, ks, ks, generator=gen) / (cin * ks * ks) ** 0.5
    b = torch.randn(cout, generator=gen) * scale
    pad = ks // 2
    ref = F.conv2d(x.double(), Wt.double(), b.double(), stride, pad)
    f32 = F.conv2d(x, Wt, b, stride, pad)
    res = torch.randn(ref.shape, generator=gen) * scale
    return {"x": x, "W": Wt, "b": b, "res": res, "ref": ref, "f32": f32, "stride": stride, "pad": pad}


def conv_want(c, with_res, relu):
    """(float64 reference, float32 floor) of a case with the residual / ReLU of the epilogue."""
    want = c["ref"] + (c["res"].double() if with_res else 0)
    f32 = c["f32"].double() + (c["res"].double() if with_res else 0)
    if relu:
        want, f32 = torch.relu(want), torch.relu(f32)
    return want, maxerr(f32, want)


def stem_weights(seed=147):
    """(W [64, 3, 7, 7], bias [64]): randn / sqrt(147); a bias of both signs, eight channels at -4 (|conv| stays below 2.5 on
    images in [0, 1]: those channels are zero after the ReLU) and eight at +3."""
    gen = torch.Generator().manual_seed(seed)
    Wt = torch.randn(64, 3, 7, 7, generator=gen) / 147 ** 0.5
    b = torch.randn(64, generator=gen) * 0.3
    b[::8] = -4.0
    b[3::8] = 3.0
    return Wt, b


def stem_ref(x, Wt, b, dtype=torch.float64):
    return F.max_pool2d(torch.relu(F.conv2d(x.to(dtype), Wt.to(dtype), b.to(dtype), 2, 3)), 3, 2, 1)


def split_bound(Wt):
    """2^-25 max_co sum |W[co]|: half an fp16 subnormal quantum per activation element."""
    return 2.0 ** -25 * float(Wt.double().abs().flatten(1).sum(1).max())


# ---- CPU emulation of the split-fp16 arithmetic ---------------------------------------------------------------------------------
def split_planes(x):
    """hi = fp16(x), lo = fp16(x - hi) (round to nearest even, subnormals kept), both returned as float32."""
    hi = x.float().to(torch.float16).float()
    lo = (x.float() - hi).to(torch.float16).float()
    return hi, lo


def emulate_conv(x, Wt, b, stride, pad, acc=torch.float32):
    """What the kernels compute: activations and 256 W as fp16 (hi, lo) planes, the three products lo x hi, hi x lo, hi x hi (each
    exact in fp32) accumulated in `acc`, then acc / 256 + bias.  The order of the accumulation is torch's, not the kernels'."""
    ah, al = split_planes(x)
    wh, wl = split_planes(Wt.float() * H2_SCALE)
    c = lambda a, w: F.conv2d(a.to(acc), w.to(acc), None, stride, pad)
    y = c(al, wh) + c(ah, wl) + c(ah, wh)
    return y * (1.0 / H2_SCALE) + b.to(acc)[None, :, None, None]


def emulate_stem(x, Wt, b, acc=torch.float32):
    return F.max_pool2d(torch.relu(emulate_conv(x, Wt, b, 2, 3, acc)), 3, 2, 1)


# ---- weight images by the unit formulas of the kernels' header comments ---------------------------------------------------------
def _planes(img):
    """Flat float32 image -> fp16 [units, 8] as float64."""
    return img.contiguous().view(torch.int16).view(torch.float16).reshape(-1, 8).double()


def unpack_conv_image(img, cout, cin, ks, cbt):
    """-> (hi, lo) [cout, cin, ks, ks] float64.  16-byte unit (((half NK + kstep) 2 + blk) 2 + plane) 64 + lane, lane = 32 h + i
    holding W[64 half + 32 blk + i][k = 16 kstep + 8 h .. + 7]; k = tap CIN + cin, or, in (channel block, tap) order,
    k = (cin / 16) 144 + tap 16 + cin % 16 (k_conv_nhwc_h2, k_conv_small_h2, k_conv3x3_patch_h2)."""
    u = _planes(img)
    nk = ks * ks * cin // 16
    assert u.shape[0] == (cout // 64) * nk * 2 * 2 * 64, (u.shape, cout, cin, ks)
    co = torch.arange(cout)[:, None, None]
    ci = torch.arange(cin)[None, :, None]
    tap = torch.arange(ks * ks)[None, None, :]
    half, blk, i = co // 64, (co % 64) // 32, co % 32
    k = (ci // 16) * ks * ks * 16 + tap * 16 + ci % 16 if cbt else tap * cin + ci
    kstep, h, e = k // 16, (k % 16) // 8, k % 8
    out = []
    for plane in range(2):
        unit = (((half * nk + kstep) * 2 + blk) * 2 + plane) * 64 + 32 * h + i
        out.append(u[unit, e.expand_as(unit)].reshape(cout, cin, ks, ks))
    return out[0], out[1]


def unpack_stem_image(img):
    """-> (hi, lo) [64, 176] float64 in k order, k = 24 ky + 3 kx + c.  16-byte unit ((kstep 2 + blk) 2 + plane) 64 + lane,
    lane = 32 h + j holding W'[32 blk + j][16 kstep + 8 h .. + 7] (k_stem_h2)."""
    u = _planes(img)
    assert u.shape[0] == 11 * 2 * 2 * 64, u.shape
    co = torch.arange(64)[:, None]
    k = torch.arange(176)[None, :]
    blk, j = co // 32, co % 32
    kstep, h, e = k // 16, (k % 16) // 8, k % 8
    out = []
    for plane in range(2):
        unit = ((kstep * 2 + blk) * 2 + plane) * 64 + 32 * h + j
        out.append(u[unit, e.expand_as(unit)])
    return out[0], out[1]
