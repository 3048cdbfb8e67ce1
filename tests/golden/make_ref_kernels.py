"""Writes tests/golden/ref_kernels_<case>.npz and ref_kernels_animate.npz (copy_data_transform): what the reference's
own CUDA kernels (oracle/_ref/ref_kernels, built by `make -C oracle ref` where the reference checkout is present)
compute, stage by stage, on the inputs of the cases of tests/test_reference_kernels.py, recorded with the SHA-256 of
each stage's inputs and what the run reported (shared-memory overrun, schedule dependence).  Arrays up to 16 KiB are
stored whole, larger ones as a SHA-256 and a seeded sample.  tests/test_reference_kernels.py compares the oracle and the product with these records, and the
live binary where it is built.
"shadowsyn" is case A of tests/test_shadow_synthetic.py (synthetic rays and triangles): the stages of the shadow pass alone.
"buildsyn" is the perspective and the spherical boundary family of tests/test_grid_build_synthetic.py: the count, slab and
fill kernels of the two grid builds alone.
"shadesyn" is the synthetic g-buffer of tests/test_shade_synthetic.py: lambertian_shade + shadow_kernel and spot_shade alone,
on every pixel in front of its undefined-cast rows.
Usage: python tests/golden/make_ref_kernels.py [case ...]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import oracle_lib as O  # noqa: E402
import test_reference_kernels as T  # noqa: E402

SHADOWSYN = "shadowsyn"  # = test_shadow_synthetic.RECORD (imported only when that record is written)
BUILDSYN = "buildsyn"  # = test_grid_build_synthetic.RECORD (likewise)
SHADESYN = "shadesyn"  # = test_shade_synthetic.RECORD (likewise)

if not O.ref_kernels_live():
    sys.exit("oracle/_ref/ref_kernels is not built from the driver in the tree (make -C oracle ref)")


def write_record(name, ins, outs, stages, reported):
    """One record: the outputs of `stages` (whole or SHA-256 and sample), the SHA-256 of every stage's inputs, and what
    the run of the `reported` stages reported."""
    rec = T.record_of(name, {st: {k: outs[st][k] for k in T.STAGE_OUTPUTS[st]} for st in stages})
    for st, i in ins.items():
        rec[st + "/input_sha"] = np.array(T.input_sha(i))
    for st in reported:
        for k in T.REPORTS:
            if k in outs[st]:
                rec["%s/report/%s" % (st, k)] = np.int64(outs[st][k][0])
    path = os.path.join(HERE, "ref_kernels_%s.npz" % name)
    np.savez_compressed(path, **rec)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes",
          {k.split("/")[0]: int(v) for k, v in rec.items() if "/report/" in k and "overrun_bytes" in k})


for name in (sys.argv[1:] or sorted(T.CASES) + [SHADOWSYN, BUILDSYN, SHADESYN]):
    if name == BUILDSYN:
        import test_grid_build_synthetic as B

        assert B.RECORD == BUILDSYN
        ins = B.ref_stage_inputs(O)
        raw = {st: T.run_reference(name, st, ins[st]) for st in B.REF_STAGES}
        outs = {st: dict(raw[st], **B.pinned(O, st, raw[st])) for st in B.REF_STAGES}
        write_record(name, ins, outs, B.REF_STAGES, B.REF_STAGES)
    elif name == SHADESYN:
        import test_shade_synthetic as SH

        assert SH.RECORD == SHADESYN
        ins = SH.ref_stage_inputs(O)
        raw = {st: O.run_ref_kernels(st, **ins[st]) for st in SH.REF_STAGES}
        outs = {st: dict(raw[st], **SH.pinned(st, raw[st])) for st in SH.REF_STAGES}
        write_record(name, ins, outs, SH.REF_STAGES, SH.REF_STAGES)
    elif name == SHADOWSYN:
        import test_shadow_synthetic as S

        assert S.RECORD == SHADOWSYN
        ins = S.ref_stage_inputs(O)
        raw = {st: O.run_ref_kernels(st, **ins[st]) for st in S.REF_STAGES}
        outs = {st: dict(raw[st], **S.pinned(O, st, raw[st])) for st in S.REF_STAGES}
        write_record(name, ins, outs, S.REF_STAGES, S.REF_STAGES)
    else:
        ins, outs = T.all_outputs(name, lambda st, i: T.run_reference(name, st, i))
        write_record(name, ins, outs, T.STAGE_OUTPUTS, T.REPORTED)
rec = {}
_, verts, orig, off, size = T.animate_inputs()
for i, rot in enumerate(T.ANIMATE_ROTS):
    ins = dict(verts=verts, orig=orig, offset=off, rot=float(np.float32(rot)))
    rec["%d/input_sha" % i] = np.array(T.input_sha(ins))
    rec["%d/verts/sha" % i] = np.array(T.array_sha(O.run_ref_kernels("animate", **ins)["verts"]))
np.savez_compressed(os.path.join(HERE, "ref_kernels_animate.npz"), **rec)
print("wrote ref_kernels_animate.npz")
