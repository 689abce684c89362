// ref_synth_gf.cc -- SYNTHETIC ZK fixtures over GF(2^128) from the real reference (build container only): the program of
// ref_synth_p256.cc over GF2_128<> / GF2_128_ID, with 16-byte elements (two bytes for a subfield element on the wire), the
// LCH14 Reed-Solomon factory of ref_flatsha.cc and the case table under REF_SYNTH_GF2_128 there (wide, odd, funnel, tall,
// long), subfield-valued inputs below begin_full_field() and the run structure of the opened columns in the record.
//
//   gen_synth_gf <case> <outdir>  ->  <outdir>/synth_gf_<case>.{lfc1,w,json}
//   gen_synth_gf --list           ->  the case names
// oracle/gen_synth_p256_fixtures.py gf compresses the two binary files and collects the records in
// tests/golden/synth_gf.json (tests/test_zk_gf_synth.py).
#define REF_SYNTH_GF2_128 1
#include "ref_synth_p256.cc"
