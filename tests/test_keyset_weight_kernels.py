"""CPU-only: the kernel of the stake weights over a registered key set exists in the built library and (a wave per group, eight
64-bit accumulators per lane behind a fully unrolled loop over the columns) keeps everything in registers.  The feature adds no
fold or pack kernel: the table is transposed by the host, invalid keys are masked inside k_ks_weight, and the registration with
proofs extends k_ks_register."""
from tests.library_support import scratch_bytes

KW_KERNELS = ("k_ks_weight", "k_ks_register")


def test_keyset_weight_kernels_built_and_their_scratch():
    scratch = scratch_bytes()
    missing = [k for k in KW_KERNELS if k not in scratch]
    assert not missing, missing
    assert scratch["k_ks_weight"] == 0, "scratch bytes per lane in k_ks_weight: %d" % scratch["k_ks_weight"]
