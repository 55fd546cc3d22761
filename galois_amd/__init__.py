"""
galois_amd -- an MI355X (gfx950) finite-field engine behind the galois.GF / FieldArray / ntt / ReedSolomon surface.

Scope: element-wise field ufuncs, np.fft.fft/ifft + ntt/intt, ReedSolomon encode/detect/decode.
All data-path work runs in hand-written HIP kernels reached through the C-ABI of include/galois_amd.h; there is no
CPU arithmetic path (importing the package without the built library raises ImportError).
"""
from . import _lib as _lib_module

_lib_module.lib()  # fail loudly if the HIP extension has not been built

from ._array import FieldArray  # noqa: E402
from ._factory import GF, Field  # noqa: E402
from ._ntt import ntt, intt  # noqa: E402
from ._codes import BCH, ReedSolomon  # noqa: E402
from ._poly import Poly, berlekamp_massey  # noqa: E402
from ._numtheory import matlab_primitive_poly, conway_poly, primitive_poly  # noqa: E402
from ._polysearch import (  # noqa: E402
    irreducible_poly, irreducible_polys, primitive_polys, is_irreducible_batched, is_primitive_batched,
)
from ._polydiv import poly_divmod_batched, poly_powmod_batched  # noqa: E402
from ._polygcd import gcd, egcd, lcm, prod, poly_gcd_batched, poly_egcd_batched, gcd_max_terms  # noqa: E402
from ._polyfactor import factors  # noqa: E402  (also gives Poly its factorisation methods)
from ._polyroots import poly_roots_batched, roots_max_terms  # noqa: E402  (also gives Poly its roots() and Roots())
from ._lagrange import lagrange_poly, lagrange_poly_batched, lagrange_max_points, crt  # noqa: E402
from ._lfsr import FLFSR, GLFSR, lfsr_step_batched, lfsr_max_order  # noqa: E402
from ._polyelem import (  # noqa: E402
    is_primitive_element, primitive_element, primitive_elements, is_normal_element, normal_element, normal_elements,
    is_primitive_element_batched, is_normal_element_batched,
)
from ._integers import (  # noqa: E402
    primes, kth_prime, prev_prime, next_prime, random_prime, mersenne_exponents, mersenne_primes, fermat_primality_test,
    miller_rabin_primality_test, legendre_symbol, jacobi_symbol, kronecker_symbol, perfect_power, trial_division, pollard_p1,
    pollard_rho, divisors, divisor_sigma, is_prime, is_composite, is_prime_power, is_perfect_power, is_smooth, is_powersmooth, isqrt,
    iroot, ilog, totatives, euler_phi, mobius, carmichael_lambda, is_cyclic, is_primitive_root, primitive_root, primitive_roots,
    are_coprime, is_square_free, is_prime_batched, primes_in_range, jacobi_symbol_batched, is_primitive_root_batched,
    sieve_segment_span,
)
from . import _dist as dist  # noqa: E402
from . import _linalg as linalg  # noqa: E402

GF2 = GF(2)

__all__ = [
    "FieldArray", "GF", "GF2", "Field", "ntt", "intt", "ReedSolomon", "BCH", "Poly", "berlekamp_massey", "is_prime", "factors", "primitive_root",
    "is_primitive_root", "matlab_primitive_poly", "conway_poly", "primitive_poly", "irreducible_poly", "irreducible_polys", "primitive_polys",
    "is_irreducible_batched", "is_primitive_batched", "poly_divmod_batched", "poly_powmod_batched", "gcd", "egcd", "lcm", "prod",
    "poly_gcd_batched", "poly_egcd_batched", "gcd_max_terms", "poly_roots_batched", "roots_max_terms", "lagrange_poly",
    "lagrange_poly_batched", "lagrange_max_points", "crt", "FLFSR", "GLFSR", "lfsr_step_batched", "lfsr_max_order", "dist", "linalg",
    "is_primitive_element", "primitive_element", "primitive_elements", "is_normal_element", "normal_element", "normal_elements",
    "is_primitive_element_batched", "is_normal_element_batched",
    "primes", "kth_prime", "prev_prime", "next_prime", "random_prime", "mersenne_exponents", "mersenne_primes", "fermat_primality_test",
    "miller_rabin_primality_test", "legendre_symbol", "jacobi_symbol", "kronecker_symbol", "perfect_power", "trial_division",
    "pollard_p1", "pollard_rho", "divisors", "divisor_sigma", "is_composite", "is_prime_power", "is_perfect_power", "is_smooth",
    "is_powersmooth", "isqrt", "iroot", "ilog", "totatives", "euler_phi", "mobius", "carmichael_lambda", "is_cyclic", "primitive_roots",
    "are_coprime", "is_square_free", "is_prime_batched", "primes_in_range", "jacobi_symbol_batched", "is_primitive_root_batched",
    "sieve_segment_span",
]
__version__ = "0.1.0"
