#!/usr/bin/env python3
"""Runs oracle/_ref/gen_synth_p256 (ref_synth_p256.cc: synthetic Fp256Base circuits compiled, proved and verified by the
real reference) for every case and stores the fixtures of tests/test_zk_p256_synth.py under tests/golden/:
  synth_p256_<case>.lfc1.xz  the circuit in the reference's LFC1 wire format (CircuitWriter output)
  synth_p256_<case>.w.xz     the witness, ninputs x 32-byte in-memory Elt images
  synth_p256.json            one record per case: shapes as compiled, LigeroParam, commitment root, SHA-256 of the proof
                             bytes and of every section of ZkProof::write, the reference verifier's verdict
With the argument fp128 the same for oracle/_ref/gen_synth_fp128 (ref_synth_fp128.cc, tests/test_zk_fp128_synth.py):
synth_fp128_<case>.{lfc1,w}.xz with 16-byte Elt images, synth_fp128.json; with the argument gf for oracle/_ref/gen_synth_gf
(ref_synth_gf.cc, tests/test_zk_gf_synth.py): synth_gf_<case>.{lfc1,w}.xz with 16-byte Elt images, synth_gf.json.
Data only -- no source text.  Usage: python oracle/gen_synth_p256_fixtures.py [p256|fp128|gf] [outdir]"""
import json
import lzma
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("p256", "fp128", "gf")


def case_names(gen):
    return subprocess.check_output([gen, "--list"], text=True).split()


def run_case(gen, field, name, tmpdir):
    """-> (record, lfc1 bytes, witness bytes) as the reference wrote them"""
    subprocess.check_call([gen, name, tmpdir], stdout=subprocess.DEVNULL)
    stem = os.path.join(tmpdir, "synth_%s_%s" % (field, name))
    return json.load(open(stem + ".json")), open(stem + ".lfc1", "rb").read(), open(stem + ".w", "rb").read()


def main(field, out):
    gen = os.path.join(HERE, "_ref", "gen_synth_" + field)
    recs = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in case_names(gen):
            rec, lfc1, w = run_case(gen, field, name, tmp)
            assert rec["reference_verifier_accepts"] is True, name
            recs.append(rec)
            for ext, data in ((".lfc1.xz", lfc1), (".w.xz", w)):
                with open(os.path.join(out, "synth_%s_%s%s" % (field, name, ext)), "wb") as f:
                    f.write(lzma.compress(data, preset=9 | lzma.PRESET_EXTREME))
    with open(os.path.join(out, "synth_%s.json" % field), "w") as f:
        f.write("{\"cases\": [\n" + ",\n".join(json.dumps(r) for r in recs) + "\n]}\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    field = args.pop(0) if args and args[0] in FIELDS else "p256"
    main(field, args[0] if args else os.path.join(os.path.dirname(HERE), "tests", "golden"))
