-- A weighted, masked Laplacian with per-pixel weights, a Param, Exclude and two unknown channels: an energy no hand-written plugin knows.
-- Written for this repo's tests (test_gpu_frontend.py, test_gpu_generated_kernels.py).
local W,H = Dims("W","H")
Inputs {
    X = Unknown(thallo_float2,{W,H},0),
    A = Array(thallo_float2,{W,H},1),
    Wt = Array(float,{W,H},2),
    Mask = Array(float,{W,H},3),
    w_fit = Param(float,4)
}
UsePreconditioner(true)
local x,y = W(),H()
X:Exclude(Not(eq(Mask(x,y),0)))
local function edge(dx,dy)
    return Select(InBounds(x+dx,y+dy), Wt(x,y)*(X(x,y) - X(x+dx,y+dy)), 0)
end
r = Residuals {
    fit = w_fit*(X(x,y) - A(x,y)),
    regx = edge(1,0),
    regy = edge(0,1)
}
