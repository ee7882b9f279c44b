-- An index map AND Exclude on the same unknown: the tie residual reaches X through the Sparse map nb, and excluded entries of X are constants -- their
-- slots in the residual's index evaluation are -1 (absent) and must receive no scatter on any lowering.  Linear.  Written for this repo's tests.
local N = Dims("N")
Inputs {
    X    = Unknown(thallo_float, {N}, 0),
    A    = Array(thallo_float, {N}, 1),
    Mask = Array(float, {N}, 2),
    nb   = Sparse({N}, {N}, 3)
}
UsePreconditioner(true)
local i = N()
X:Exclude(Not(eq(Mask(i), 0)))
Residuals {
    fit = X(i) - A(i),
    tie = 0.5 * (X(i) - X(nb(i)))
}
