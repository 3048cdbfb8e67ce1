"""Writes tests/golden/ref_objdump_<scene>.npz: what the reference's own OBJ/MTL parser (oracle/_ref/ref_objdump,
built by `make -C oracle ref` where the reference checkout is present) reads from the scene files of
tests/test_host.py, recorded with the SHA-256 of the OBJ it read.  tests/test_host.py compares the product's loader
with these records, and with the parser itself where it is built.
Usage: python tests/golden/make_ref_objdump.py"""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import oracle_lib as O  # noqa: E402
import test_host as T  # noqa: E402
import ugrt  # noqa: E402

if not os.path.exists(O.REF_OBJDUMP):
    sys.exit("oracle/_ref/ref_objdump is not built (make -C oracle ref)")
for name in T.REF_SCENES:
    with tempfile.TemporaryDirectory() as d:
        obj, _ = T.ref_scene(ugrt, name, d)
        out = os.path.join(d, "dump.bin")
        subprocess.run([O.REF_OBJDUMP, os.path.basename(obj), out], cwd=d, check=True, capture_output=True)
        rec = T.parse_ref_dump(open(out, "rb").read())
        rec["obj_sha256"] = np.array(hashlib.sha256(open(obj, "rb").read()).hexdigest())
    path = os.path.join(HERE, "ref_objdump_%s.npz" % name)
    np.savez_compressed(path, **rec)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")
