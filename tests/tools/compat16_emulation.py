"""CPU emulation (checker-side tool, never the product) of the GUARDED 16-bit compat cache: per
(pair, layer) the attention streams c as 16-bit fixed point, c16 = rint(65535 c) / 65535, exactly where the device-side guard
lets the layer through, and the fp32 c where it trips.

The guard is the one the fp8 cross products already use (gmf_pack.cpp pv_guard_threshold; PvGuard): the layer's score bound
    Z = (1.02 |Wq|_2 F + |bq|) (1.02 |Wk|_2 F + |bk|) / sqrt(C),       F = max row |f|
against a limit.  The fp8 products keep their limit of 1024; the cache format is decided at C16_SCORE (a power of two <= 1024).

The whole encoder runs in fp64 around an emulation of the shipped operand arithmetic (mx_cross_emulation.py `fp8x_g`, the
unfolded default; kv_fold_emulation.py `foldp_g`, the folded default of large grids), whose helpers this file imports.  Per
input it prints max |logit - fp64 logit| of the fp32 oracle, of both shipped forms on the fp32 cache, and of both forms under
the guarded 16-bit cache at every candidate limit, with the number of layers that stream 16 bits in brackets and the layers'
score bounds Z on a line of their own.  It asserts the one contract of the default numerics on every entry at C16_SCORE:
    |logit - fp64| <= 1.5 x (fp32 oracle vs fp64) + 2e-5,      and <= 1e-4 on 3DMatch-shape inputs.

    python tests/tools/compat16_emulation.py            # the whole table (profiles/compat16_emulation.txt)
    python tests/tools/compat16_emulation.py quick      # one seed per input family, the chosen limit only"""
import math, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_cross_emulation as E
import kv_fold_emulation as KF
from mx_cross_emulation import O, synthetic

C16_SCORE = 1024.0                                   # the limit the library ships for the cache format (see the table)
CANDIDATES = [1024.0, 512.0, 256.0, 128.0, 64.0, 32.0]
score_log = []


def layer_score(feat, Wq, bq, Wk, bk):
    """the guard's score bound of this layer, as the packer and the kernels form it"""
    C = feat.shape[-1]
    sq = 1.02 * float(torch.linalg.matrix_norm(Wq.reshape(C, C), 2)); sk = 1.02 * float(torch.linalg.matrix_norm(Wk.reshape(C, C), 2))
    F = float(feat.norm(dim=-1).max())
    return (sq * F + float(bq.norm())) * (sk * F + float(bk.norm())) / math.sqrt(C)


def c16(compat):
    """c as the 16-bit cache holds it (k_compat_build<2>): the fp32 c, rint(65535 c) in fp32, read back exactly"""
    c = compat.float()
    return (torch.round(c * 65535.0) / 65535.0).double()


def make_c16(base, limit):
    """`base` (a shipped form) with the 16-bit c in the layers whose score bound is within `limit`"""
    def sc_attention(feat, compat, Wq, bq, Wk, bk, Wv, bv):
        z = layer_score(feat, Wq, bq, Wk, bk)
        score_log.append(z)
        return base(feat, c16(compat) if z <= limit else compat, Wq, bq, Wk, bk, Wv, bv)
    return sc_attention


ROWS = [  # (label, kind, N, seeds, conditioned weights, 3DMatch-shape: the literal 1e-4 gate applies, asserted)
    ("3dmatch N=1000", "3dmatch", 1000, [1000, 1001, 1002, 1003], False, True, True),
    ("3dmatch N=2000", "3dmatch", 2000, [7, 8], False, True, True),
    ("kitti stress N=700", "kitti", 700, [83, 84, 85], False, False, True),
    ("kitti stress N=2000 (F22)", "kitti", 2000, [84, 0], False, False, True),
    ("kitti --cond N=700", "kitti", 700, [83, 84], True, False, True),
    # Printed, not asserted: on this input the emulation of the SHIPPED fp8 form on the fp32 cache is itself outside the bound (7.5e-5
    # against 4.6e-5), because the emulated P planes are coarser than the kernel's (profiles/r04_kitti_weight_sets.txt: the HIP path
    # measures 1.6e-5 where this arithmetic says 6.4e-5).  What the row shows is the step the 16-bit c adds to it: below 5e-6.
    ("kitti --cond N=2000 (F22; not asserted, see ROWS)", "kitti", 2000, [84], True, False, False),
]


def main():
    quick = "quick" in sys.argv[1:]
    limits = [C16_SCORE] if quick else CANDIDATES
    sd0 = synthetic.seeded_state_dict(synthetic.pointdsc_shapes(6, 12, 128), seed=7)
    exact = O.sc_attention
    forms = (("fp8x_g", lambda: E.make_attention("fp8x_g")), ("foldp_g", lambda: KF.make_fold(True)))
    rel = {lim: 0.0 for lim in limits}               # the largest entry relative to its bound, per limit
    bad = []
    for label, kind, N, seeds, cond, gate, asserted in ROWS:
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
            bound = min(1.5 * floor + 2e-5, 1e-4) if gate else 1.5 * floor + 2e-5

            def run(att):
                O.sc_attention = att
                try:
                    got = O.classifier(sd64, O.encoder(sd64, b64["corr_pos"], compat32.double(), b64["p_tokens"], b64["q_tokens"], 12))
                finally:
                    O.sc_attention = exact
                    E.guard_log.clear()
                return float((got - truth).abs().max())

            print(f"  seed {seed}: fp32 oracle {floor:.2e}   bound {bound:.2e}")
            for name, make in forms:
                row = [f"    {name}: fp32 cache {run(make()):.2e}"]
                for lim in limits:
                    score_log.clear()
                    err = run(make_c16(make(), lim))
                    n16 = sum(z <= lim for z in score_log)
                    row.append(f"c16<={lim:g} {err:.2e} [{n16}] ({err / bound:.2f})")
                    if asserted:
                        rel[lim] = max(rel[lim], err / bound)
                    if asserted and lim == C16_SCORE and err > bound:
                        bad.append((label, seed, name, err, bound))
                print("   ".join(row), flush=True)
            print("    score bound Z per layer (last form): " + " ".join(f"{z:.3g}" for z in score_log), flush=True)
    for lim in limits:
        print(f"limit {lim:g}: largest asserted entry relative to its bound: {rel[lim]:.3f}")
    assert not bad, bad
    print(f"at the limit {C16_SCORE:g}: every asserted entry within 1.5 x (fp32 oracle vs fp64) + 2e-5; every 3DMatch-shape entry within 1e-4")


if __name__ == "__main__":
    main()
