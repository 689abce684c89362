"""What the seven instantiations of K1's 1024 x 4 tile kernels (csrc/fft.hip) compile to for gfx950, in one table.  The three
kernel bodies share their rounds (the t4_round* helpers), so an edit to a helper moves all seven; the figures are those of the
commit before the rounds were shared, and nothing may rise above them.  The per-feature ceilings of the older tests
(test_fp_tile_arith.py ... test_fp_tile_mul_carries.py) record how each count was reached."""
import pytest

import fft_isa

ARGS3 = "I8Fp128OpsLb%dELb%dEEv8TilePlanPK5elt_tjS4_j"
ARGS2 = "I8Fp128OpsLb%dEEv8TilePlanPK5elt_tjS4_j"
# kernel: (VALU <=, VGPRs <=, LDS instructions ==, global loads + stores ==)
PINS = {
    "_Z18fp_fft_tile_1024x4" + ARGS3 % (0, 1): (3179, 115, 65, 25),  # pass A, one-tile launch, with the inter-pass product
    "_Z18fp_fft_tile_1024x4" + ARGS3 % (1, 0): (2744, 80, 65, 17),  # pass B
    "_Z26fp_fft_tile_1024x4_persistI8Fp128OpsEv8TilePlanPK5elt_tjS4_jj": (3209, 128, 68, 25),  # pass A, XCD-aware order / tile loop
    "_Z22fp_fft_tile_1024x4_tws" + ARGS2 % 0: (2617, 71, 65, 17),  # pass A of the default pair
    "_Z22fp_fft_tile_1024x4_tws" + ARGS2 % 1: (3079, 86, 65, 25),  # pass B of the default pair, with the inter-pass product
    "_Z28fp_fft_tile_1024x4_tws_canon" + ARGS2 % 0: (2725, 85, 65, 17),
    "_Z28fp_fft_tile_1024x4_tws_canon" + ARGS2 % 1: (3143, 86, 65, 25),
}


@pytest.mark.parametrize("name", PINS)
def test_tile_kernel_isa_pins(name):
    valu_max, vgpr_max, n_ds, n_global = PINS[name]
    k = fft_isa.kernel(name)
    figures = (fft_isa.valu(name), k.desc["next_free_vgpr"], sum(op.startswith("ds_") for op in k.ops),
               sum(op.startswith("global_") for op in k.ops))
    print(name, "VALU, VGPRs, ds, global:", figures, "scratch:", k.desc["private_segment_fixed_size"])
    assert k.desc["private_segment_fixed_size"] == 0
    assert not any(op.startswith(("scratch_", "buffer_", "flat_")) for op in k.ops)
    assert figures[0] <= valu_max and figures[1] <= vgpr_max, (figures, PINS[name])
    assert figures[2:] == (n_ds, n_global), (figures, PINS[name])
