"""The multi-limb fields of tests/test_limb_params_host.py and tests/test_gpu_limb_edges.py: every (limb count, arithmetic kind)
pair of csrc/gfa_wide.hip (2 limbs) and csrc/gfa_big.hip (4 / 8 / 16 limbs), each at moduli that fill the top limb, leave it nearly
empty, or sit on a limb boundary.  Primality and irreducibility of every modulus are checked by test_limb_params_host.py with
a Miller-Rabin and a Rabin test written there on Python integers.

The binomials x^t - a are irreducible over GF(p) by the binomial criterion: every prime factor of t divides ord(a) but not
(p - 1) / ord(a), and p = 1 mod 4 when 4 | t.  "- a" is the coefficient p - a."""
from oracle.wide_oracle import WideOracle


def _bits(*exps):
    return sum(1 << e for e in exps)


def _binomial(p, t, a):
    return [1] + [0] * (t - 1) + [p - a]  # x^t - a, degree t .. 0


P32 = 2**32 - 5  # the largest characteristic of an extension field (p < 2^32)

# tag -> characteristic, degree, modulus (None / bit mask of a binary polynomial / coefficients of degree m .. 0), limbs per element
FIELDS = {
    # prime fields
    "p_2e64_p13": dict(p=2**64 + 13, m=1, irr=None, nl=2),             # smallest two-limb prime: high limb 1, low limb 13
    "p_2e127_m1": dict(p=2**127 - 1, m=1, irr=None, nl=2),             # bit 127 clear, all lower bits set
    "p_2e128_m159": dict(p=2**128 - 159, m=1, irr=None, nl=2),         # full width: the carry-out and t2 branches
    "p_2e129_m25": dict(p=2**129 - 25, m=1, irr=None, nl=4),           # smallest k-limb size
    "p_2e256_m189": dict(p=2**256 - 189, m=1, irr=None, nl=4),         # full width on 4 limbs
    "p_secp256k1": dict(p=2**256 - 2**32 - 977, m=1, irr=None, nl=4),  # full width on 4 limbs
    "p_2e257_m93": dict(p=2**257 - 93, m=1, irr=None, nl=8),           # first 8-limb prime, upper limbs nearly empty
    "p_p384": dict(p=2**384 - 2**128 - 2**96 + 2**32 - 1, m=1, irr=None, nl=8),  # 8 limbs, two empty
    "p_2e512_m569": dict(p=2**512 - 569, m=1, irr=None, nl=8),         # full width on 8 limbs
    "p_2e513_m445": dict(p=2**513 - 445, m=1, irr=None, nl=16),        # first 16-limb prime
    "p_2e1024_m105": dict(p=2**1024 - 105, m=1, irr=None, nl=16),      # full width on 16 limbs
    # binary fields
    "gf2e64": dict(p=2, m=64, irr=_bits(64, 4, 3, 1, 0), nl=2),        # m = 64: the smallest order of the two-limb class
    "gf2e129": dict(p=2, m=129, irr=_bits(129, 5, 0), nl=4),           # smallest k-limb degree
    "gf2e192": dict(p=2, m=192, irr=_bits(192, 7, 2, 1, 0), nl=4),     # m a multiple of 64 below 64 NL: a whole limb is cleared
    "gf2e320": dict(p=2, m=320, irr=_bits(320, 4, 3, 1, 0), nl=8),     # the same on 8 limbs
    "gf2e512": dict(p=2, m=512, irr=_bits(512, 8, 5, 2, 0), nl=8),     # m = 64 NL on 8 limbs: implicit top bit
    "gf2e576": dict(p=2, m=576, irr=_bits(576, 13, 4, 3, 0), nl=16),   # first 16-limb binary field, m a multiple of 64
    "gf2e1024": dict(p=2, m=1024, irr=_bits(1024, 19, 6, 1, 0), nl=16),  # m = 64 NL on 16 limbs
    # extension fields of odd characteristic
    "gf17e16": dict(p=17, m=16, irr=_binomial(17, 16, 3), nl=2),           # largest two-limb degree
    "gf65521e8": dict(p=65521, m=8, irr=_binomial(65521, 8, 17), nl=2),    # order of 128 bits: top limb full
    "gf17e32": dict(p=17, m=32, irr=_binomial(17, 32, 3), nl=4),           # the largest k-limb degree (BMAXD)
    "gfP32e5": dict(p=P32, m=5, irr=_binomial(P32, 5, 2), nl=4),           # largest characteristic
    "gfP32e10": dict(p=P32, m=10, irr=_binomial(P32, 10, 2), nl=8),        # extension kind on 8 limbs
    "gfP32e25": dict(p=P32, m=25, irr=_binomial(P32, 25, 2), nl=16),       # extension kind on 16 limbs
}
TAGS = list(FIELDS)
FULL_WIDTH_PRIMES = [t for t, f in FIELDS.items() if f["m"] == 1 and f["p"].bit_length() == 64 * f["nl"]]
assert FULL_WIDTH_PRIMES == ["p_2e128_m159", "p_2e256_m189", "p_secp256k1", "p_2e512_m569", "p_2e1024_m105"]


def kind(f):
    return "prime" if f["m"] == 1 else "binary" if f["p"] == 2 else "extension"


def irr_coeffs(f):
    """Coefficients of the modulus, degree m .. 0 (None for a prime field)."""
    if f["m"] == 1:
        return None
    irr, m = f["irr"], f["m"]
    return list(irr) if isinstance(irr, list) else [(irr >> (m - i)) & 1 for i in range(m + 1)]


def irr_int(f):
    """The modulus as the integer sum c_i p^i, the form galois_amd.GF stores and wide_params / big_params take."""
    v = 0
    for c in irr_coeffs(f):
        v = v * f["p"] + c
    return v


def oracle(tag):
    f = FIELDS[tag]
    return WideOracle(f["p"], f["m"], irr_coeffs(f))


def make_field(tag):
    """The field class with an explicit primitive element (2, or the element x: any legal non-zero value -- no arithmetic kernel
    reads it) and verify=False, so that no construction factors q - 1 to verify it."""
    import galois_amd as ga

    f = FIELDS[tag]
    if f["m"] == 1:
        return ga.GF(f["p"], primitive_element=2, verify=False)
    return ga.GF(f["p"], f["m"], irreducible_poly=f["irr"], primitive_element=f["p"], verify=False)
