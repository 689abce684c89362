"""Child process of test_sumcheck_drivers.py: the tuning switches are read once per process, so every combination
gets its own.  Proves the fixture circuit with the fixture's RandomEngine / transcript seed, requires the wire bytes
of the reference and that the verifier accepts them.
Usage: zk_mode_child.py <nb> [fp128] | sig | synth:<case> | synthfp:<case>
  <nb> [fp128]    the flatsha circuit of nb blocks over GF(2^128), or over Fp128 (nb = 1 only)
  sig             the mdoc signature circuit over Fp256Base
  synth:<case>    a synthetic Fp256Base circuit of test_zk_p256_synth.py
  synthfp:<case>  a synthetic Fp128 circuit of test_zk_fp128_synth.py
The synthetic cases carry their own rate, query count and block_enc; witness rows are 4 limbs over Fp256Base, else 2."""
import hashlib, json, lzma, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gpu_util as G
import ligero_fixture as lf

gold = os.path.join(ROOT, "tests", "golden")
sig = sys.argv[1] == "sig"  # the mdoc signature circuit over Fp256Base (32-byte elements, csrc/zk256.hip)
synth = sys.argv[1].startswith("synth:")  # a synthetic Fp256Base circuit of test_zk_p256_synth.py, with its own rate / query count
synthfp = sys.argv[1].startswith("synthfp:")  # a synthetic Fp128 circuit of test_zk_fp128_synth.py, likewise (16-byte elements, csrc/zk.hip)
rate, nreq = 7, 132
if sig:
    stem = "mdoc_sig"
    info = json.load(open(os.path.join(gold, "mdoc.json")))["sig"]
    be = info["block_enc"]
elif synth or synthfp:
    fam, case = ("synth_p256", sys.argv[1][6:]) if synth else ("synth_fp128", sys.argv[1][8:])
    stem = fam + "_" + case
    info = {r["case"]: r for r in json.load(open(os.path.join(gold, fam + ".json")))["cases"]}[case]
    rate, nreq, be = info["rate"], info["nreq"], info["block_enc_arg"]
else:
    nb = int(sys.argv[1])
    fp = len(sys.argv) > 2 and sys.argv[2] == "fp128"
    stem = ("flatsha_fp_nb%d" if fp else "flatsha_nb%d") % nb
    info = json.load(open(os.path.join(gold, stem + ".json")))
    be = 0
raw = lzma.decompress(open(os.path.join(gold, stem + ".lfc1.xz"), "rb").read())
W = np.frombuffer(lzma.decompress(open(os.path.join(gold, stem + ".w.xz"), "rb").read()), dtype=np.uint64).reshape(-1, 4 if sig or synth else 2).copy()
pkg, gpu = G.pkg, G.gpu()
circ = pkg.Circuit(gpu, raw)
zk = pkg.ZkProver(gpu, circ, rate, nreq, be)
for rep in range(2):  # twice: the second run reuses cached buffers and the warmed-up drivers
    ts = pkg.FsTranscript(b"test")
    zk.commit(W, lf.LcgRng(100).bytes, ts)
    assert zk.prove(W, ts), "prove failed"
    wire = zk.wire()
    ts.close()
    assert len(wire) == info["zk_wire_bytes"] and hashlib.sha256(wire).hexdigest() == info["zk_wire_sha256"], "wire differs from the reference"
ts = pkg.FsTranscript(b"test")
ok, why = pkg.zk_verify(gpu, circ, wire, W[:circ.info.npub_in], ts, rate, nreq, be)
ts.close()
assert ok, why
print("OK", stem)
