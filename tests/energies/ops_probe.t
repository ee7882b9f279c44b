-- The generated prelude's number functions one by one: one unknown image per function and ONE single-access residual f(X(i)) + B(i) per image, so that
-- r_i = -f'(x_i) (f(x_i) + b_i) and diag_i = f'(x_i)^2 are elementwise observables of f and f' (tests/test_gpu_prelude_functions.py).  Written for this repo's tests.
local N = Dims("N")
Inputs {
    Xadd  = Unknown(thallo_float, {N}, 0),
    Xsub  = Unknown(thallo_float, {N}, 1),
    Xmul  = Unknown(thallo_float, {N}, 2),
    Xdiv  = Unknown(thallo_float, {N}, 3),
    Xrcp  = Unknown(thallo_float, {N}, 4),
    Xsqrt = Unknown(thallo_float, {N}, 5),
    Xsin  = Unknown(thallo_float, {N}, 6),
    Xcos  = Unknown(thallo_float, {N}, 7),
    Xabs  = Unknown(thallo_float, {N}, 8),
    Xpow  = Unknown(thallo_float, {N}, 9),
    Xsel  = Unknown(thallo_float, {N}, 10),
    B     = Array(thallo_float, {N}, 11),
    Bz    = Array(thallo_float, {N}, 12),
    C     = Array(thallo_float, {N}, 13),
    pw    = Param(float, 14)
}
UsePreconditioner(false)
local i = N()
Residuals {
    e_add  = (Xadd(i) + C(i)) + B(i),
    e_sub  = (C(i) - Xsub(i)) + B(i),
    e_mul  = Xmul(i) * C(i) + B(i),
    e_div  = Xdiv(i) / C(i) + B(i),
    e_rcp  = C(i) / Xrcp(i) + B(i),
    e_sqrt = sqrt(Xsqrt(i)) + B(i),
    e_sin  = sin(Xsin(i)) + Bz(i),
    e_cos  = cos(Xcos(i)) + Bz(i),
    e_abs  = abs(Xabs(i)) + Bz(i),
    e_pow  = pow(Xpow(i), pw) + B(i),
    e_sel  = Select(greater(Xsel(i), C(i)), Xsel(i) * Xsel(i), 2 * Xsel(i)) + B(i)
}
