"""CPU emulation (checker-side tool, never the product) of the "kv_fold" form of the spatial-consistency attention
(PointDSC.py:56-64): keys = values = the layer input f, with the K projection folded into the query side and
the V projection folded behind the normalisation -

    s_ij = q'_i . (Wk f_j + bk)            = f_j . q~_i + beta_i,     q~ = (Wk^T Wq') f + Wk^T bq',   beta = (Wq'^T bk) . f + bk . bq'
    sum_j p_ij (Wv f_j + bv)               = Wv (sum_j p_ij f_j) + bv                                  (a softmax row sums to 1)

in the PRECOMPOSED form the library ships: the composed matrices are formed in fp64, rounded once to fp32 and split into fp16
planes of 256 W (gmf_pack.cpp), q~ and beta are fp32 numbers, the key and value tiles are the split-fp16 planes of f (under the
guard: the e4m3 cross planes of f, one scale per (row, 32 channels) for the keys and per (feature, 32-key tile) for the values),
and Wv, bv act on the normalised fp32 output (in the library through the composed first layer of fc_message).

The whole encoder runs in fp64 except the two contractions, as in mx_cross_emulation.py, whose helpers this file imports.  Per
input it prints max |logit - fp64 logit| of
    the fp32 oracle | split3 (the shipped f16 form) | foldp3 (the fold, f16 form) | fp8x_g (the shipped guarded fp8 form) | foldp_g
and asserts the two contracts on every fold entry: <= 1.5 x (fp32 oracle vs fp64) + 2e-5, and <= 1e-4 on 3DMatch-shape inputs.

    python tests/tools/kv_fold_emulation.py            # the whole table (profiles/kv_fold_emulation.txt)
    python tests/tools/kv_fold_emulation.py quick      # one row per input family"""
import math, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_cross_emulation as E
from mx_cross_emulation import O, synthetic, f16, e4m3, tiles, _blk32


def split_w(W):
    """a weight matrix as the packer stores it: fp32, then fp16 planes of 256 W (hi + lo)"""
    w = W.float().double() * 256.0
    hi = f16(w)
    return (hi + f16(w - hi)) / 256.0


def split_x(x):
    """an activation as the kernels multiply it: fp32, then two fp16 planes"""
    x = x.float().double()
    hi = f16(x)
    return hi + f16(x - hi)


def make_fold(guarded_form):
    split3 = E.make_attention("split3")

    def sc_attention(feat, compat, Wq, bq, Wk, bk, Wv, bv):
        C = feat.shape[-1]
        Wq2, Wk2, Wv2 = Wq.reshape(C, C), Wk.reshape(C, C), Wv.reshape(C, C)
        f = feat.float().double()                                  # the layer input is an fp32 image
        use_f8 = False
        if guarded_form:
            sq = 1.02 * float(torch.linalg.matrix_norm(Wq2, 2)); sk = 1.02 * float(torch.linalg.matrix_norm(Wk2, 2))
            F = float(feat.norm(dim=-1).max())
            tripped = (sq * F + float(bq.norm())) * (sk * F + float(bk.norm())) / math.sqrt(C) > E.GUARD_SCORE
            E.guard_log.append(int(tripped))
            use_f8 = not tripped
        # the composed query side (fp64 product, rounded once)
        Wqf = split_w(Wk2.t() @ Wq2)                               # q~ = Wqf f + bqf
        bqf = (Wk2.t() @ bq).float().double()
        u = (Wq2.t() @ bk).float().double()                        # beta = u . f + b0
        b0 = float((bk @ bq).float())
        qt = (split_x(f) @ Wqf.t() + bqf).float().double()
        beta = (f @ u + b0).float().double()
        qh = f16(qt); ql = f16(qt - qh)
        kh = f16(f); kl = f16(f - kh)                              # the key tile: planes of f
        s = qh @ kh.transpose(1, 2)
        if use_f8:
            s = s + _blk32(qt) @ _blk32(kl).transpose(1, 2) + _blk32(ql) @ _blk32(f).transpose(1, 2)
        else:
            s = s + qh @ kl.transpose(1, 2) + ql @ kh.transpose(1, 2)
        s = (s + beta[..., None]).float().double() / math.sqrt(C)
        z = (compat * s).float().double()
        p = torch.exp(z - z.amax(-1, keepdim=True)).float().double()
        ph = f16(p); pl = f16(p - ph)
        if use_f8:
            fix = lambda x: (x * 256.0).float().to(torch.float8_e4m3fn).double() / 256.0
            p8, pl8 = fix(p), fix(pl)
            vt, _ = tiles(f, 1); vlt, _ = tiles(kl, 1)
            v8 = e4m3(vt, 2).reshape(f.shape[0], -1, f.shape[2])[:, :f.shape[1]]
            vl8 = e4m3(vlt, 2).reshape(f.shape[0], -1, f.shape[2])[:, :f.shape[1]]
            o = (ph @ kh + p8 @ vl8 + pl8 @ v8).float().double() / (ph + pl8).sum(-1, keepdim=True)
        else:
            o = (ph @ kh + ph @ kl + pl @ kh).float().double() / p.sum(-1, keepdim=True)
        # Wv, bv behind the normalisation: the epilogue multiplies the split planes of the fp32 output
        return split_x(o) @ Wv2.t() + bv
    return sc_attention


ROWS = [  # (label, kind, N, seeds, conditioned weights, 3DMatch-shape: the literal 1e-4 gate applies)
    ("3dmatch N=1000", "3dmatch", 1000, [1000, 1001, 1002, 1003], False, True),
    ("3dmatch N=2000", "3dmatch", 2000, [7, 8], False, True),
    ("kitti stress N=700", "kitti", 700, [83, 84, 85], False, False),
    ("kitti stress N=2000", "kitti", 2000, [0], False, False),
    ("kitti --cond N=700", "kitti", 700, [83, 84], True, False),
]


def main():
    quick = "quick" in sys.argv[1:]
    sd0 = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, 12, 128), seed=7)
    exact = O.sc_attention
    schemes = (("split3", lambda: E.make_attention("split3")), ("foldp3", lambda: make_fold(False)),
               ("fp8x_g", lambda: E.make_attention("fp8x_g")), ("foldp_g", lambda: make_fold(True)))
    worst = 0.0
    bad = []
    for label, kind, N, seeds, cond, gate in ROWS:
        sigma_d = 0.1 if kind == "3dmatch" else 1.2
        sd = synthetic.kitti_conditioned(sd0) if cond else sd0
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        print(f"{label}: max |logit - fp64 logit|")
        for seed in (seeds[:1] if quick else seeds):
            b = synthetic.synthetic_batch([seed], N=N, T=196, kind=kind)
            b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in b.items()}
            compat64, _ = O.compat_matrix(b64["src_keypts"], b64["tgt_keypts"], sigma_d)
            compat32, _ = O.compat_matrix(b["src_keypts"], b["tgt_keypts"], sigma_d)
            truth = O.classifier(sd64, O.encoder(sd64, b64["corr_pos"], compat64, b64["p_tokens"], b64["q_tokens"], 12))
            ref32 = O.classifier(sd, O.encoder(sd, b["corr_pos"], compat32, b["p_tokens"], b["q_tokens"], 12))
            floor = float((ref32.double() - truth).abs().max())
            row = [f"seed {seed}: fp32 oracle {floor:.2e}"]
            try:
                for name, make in schemes:
                    O.sc_attention = make()
                    got = O.classifier(sd64, O.encoder(sd64, b64["corr_pos"], compat32.double(), b64["p_tokens"], b64["q_tokens"], 12))
                    err = float((got - truth).abs().max())
                    row.append(f"{name} {err:.2e}" + (f" [{sum(E.guard_log)}]" if name.endswith("_g") else ""))
                    E.guard_log.clear()
                    if name.startswith("foldp"):
                        worst = max(worst, err / (1.5 * floor + 2e-5))
                        if err > 1.5 * floor + 2e-5 or (gate and err > 1e-4):
                            bad.append((label, seed, name, err, floor))
            finally:
                O.sc_attention = exact
            print("  " + "   ".join(row), flush=True)
    print(f"largest fold entry relative to its bound 1.5 x floor + 2e-5: {worst:.3f}")
    assert not bad, bad
    print("every fold entry within 1.5 x (fp32 oracle vs fp64) + 2e-5; every 3DMatch-shape entry within 1e-4")


if __name__ == "__main__":
    main()
