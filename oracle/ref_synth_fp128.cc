// ref_synth_fp128.cc -- SYNTHETIC ZK fixtures over Fp128 from the real reference (build container only): the program of
// ref_synth_p256.cc over Fp128<> / FP128_ID, with 16-byte elements, the FFT Reed-Solomon factory of ref_flatsha.cc under
// REF_FP128 and the case table under REF_SYNTH_FP128 there (wide, odd, funnel, tall, long).
//
//   gen_synth_fp128 <case> <outdir>  ->  <outdir>/synth_fp128_<case>.{lfc1,w,json}
//   gen_synth_fp128 --list           ->  the case names
// oracle/gen_synth_p256_fixtures.py fp128 compresses the two binary files and collects the records in
// tests/golden/synth_fp128.json (tests/test_zk_fp128_synth.py).
#define REF_SYNTH_FP128 1
#include "ref_synth_p256.cc"
