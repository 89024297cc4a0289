"""Shared by tests/test_gp_kmeans_cpu.py and tests/test_gp_kmeans.py: an fp64 torch restatement of one Lloyd step of
k-means and of the Lloyd loop of cgat_amd.kmeans_inducing_points (the reference's only choice of inducing
points is the random batch of CGAT/gaussian_process.py:223-226), the rule an fp32 assignment is held to, and the fixtures.

    step   : a_n = argmin_m |x_n - z_m|^2 (a tie to the smaller m),  counts_m = #{a_n = m},  wss_m = sum_{a_n = m} |x_n - z_m|^2,
             sums_m = sum_{a_n = m} (x_n - centroid),  centroid = mean_m z_m rounded to fp32 (what the kernel centres with)
    update : z_m <- centroid + sums_m / counts_m where counts_m > 0, rounded to fp32 (the package rounds Z between steps)
    loop   : at most `iters` steps; a step whose assignment repeats the one before it ends the loop without its update

The near-tie rule.  An fp32 evaluation cannot order two centres whose distances to a row differ by less than its own
error.  The kernel forms |x - c|^2 + |z - c|^2 - 2 (x - c).(z - c) for both, with c the fp32 centroid of Z.  Each of the
three terms is a sum of D products with relative error at most (D + 2) u of its absolute sum, u = 2^-24, the absolute
sums being |x - c|^2, |z - c|^2 and at most |x - c|^2 + |z - c|^2 (2 |ab| <= a^2 + b^2), plus one rounding each for the
two additions: at most 2 (D + 3) u (|x - c|^2 + |z - c|^2) per distance, twice that for the difference of two distances,
and a factor 2 for the rounding of x - c itself (one rounding per entry, entering every term twice):

    B_n = 8 (D + 3) 2^-24 (|x_n - cbar|^2 + max_m |z_m - cbar|^2),   cbar = mean_m z_m

With gap_n the fp64 difference between the second smallest and the smallest distance of row n: a row with gap_n > B_n
must receive the restatement's centre; any other row a centre whose fp64 distance is within B_n of the minimum; and among
bit-identical centres only the lowest index may be returned.

Nothing here touches the package under test or the GPU."""
import functools
import math

import torch

import gp_fit_cases

PARITY = 1e-4                                     # the project's criterion, of each quantity's max-norm
OFFSET = 3.0                                      # of every embedding: the centring matters
# (N, M, D) of the step cases.  `chunk_rows`: what the GPU test passes (None: the default); `ldx_pad`: a row stride D + pad
CASES = {
    "n1_m1_d1": dict(N=1, M=1, D=1),                               # the minimum
    "n31_m30_d7": dict(N=31, M=30, D=7),                           # below one tile
    "n150_m33_d5": dict(N=150, M=33, D=5, chunk_rows=64),          # three chunks, the last partial; Mp = 64
    "n300_m96_d65": dict(N=300, M=96, D=65, ldx_pad=3),            # Dp = 128, a padded row stride
    "n1100_m1024_d384": dict(N=1100, M=1024, D=384),               # two slabs, every wave owns four chunks of centres
    "n65_m129_d640": dict(N=65, M=129, D=640),                     # D = 640, more centres than rows
}
# The Lloyd fixtures: well separated clusters, M drawn as GPHead.fit draws its subset with `seed`.  The seeds were searched
# on the CPU (tests/test_gp_kmeans_cpu.py holds what the search was for): every row of every step has gap > 100 B, the
# loop makes at least two updates and converges within LLOYD_ITERS steps.
LLOYD_ITERS = 5
LLOYD_CASES = {
    "n150_m6_d5": dict(N=150, M=6, D=5, clusters=6, data_seed=1, seed=1, chunk_rows=64),
    "n300_m9_d7": dict(N=300, M=9, D=7, clusters=9, data_seed=0, seed=5),
}


def mixture(N, D, clusters, separation, generator, decay=None):
    """N rows of a Gaussian mixture with unit noise, unequal populations (weights 1 : 2 : ... : clusters) and means
    `separation` x N(0, I), offset by OFFSET; fp32.  `decay`: column j of means and noise is scaled by
    1 / sqrt(1 + j / decay), the falling spectrum of a learned embedding."""
    means = separation * torch.randn(clusters, D, generator=generator)
    w = torch.arange(1, clusters + 1, dtype=torch.float64)
    comp = torch.multinomial(w / w.sum(), N, replacement=True, generator=generator)
    rows = means[comp] + torch.randn(N, D, generator=generator)
    if decay is not None:
        rows = rows / torch.sqrt(1.0 + torch.arange(D, dtype=torch.float32) / decay)
    return OFFSET + rows


def build_inputs(N, M, D, seed=0, **_):
    """A step case: X [N, D] and centres Z [M, D] drawn from one mixture (Z independent rows of it), fp32 on the CPU."""
    g = torch.Generator().manual_seed(3000 + seed + 7 * N + 13 * M + 17 * D)
    rows = mixture(N + M, D, max(1, min(8, M // 4)), 1.0, g, decay=8.0)
    return dict(X=rows[:N].clone(), Z=rows[N:].clone())


def build_lloyd_inputs(N, M, D, clusters, data_seed=0, **_):
    """A Lloyd fixture: X [N, D] of well separated clusters and targets y [N] (a smooth function of a projection plus noise,
    as gp_fit_cases builds them), fp32 on the CPU."""
    g = torch.Generator().manual_seed(4000 + data_seed + 7 * N + 13 * M + 17 * D)
    X = mixture(N, D, clusters, 4.0, g)
    w = torch.randn(D, generator=g) / math.sqrt(D)
    t = (X - OFFSET) @ w / 4.0
    y = 3.0 + 2.0 * (torch.sin(1.3 * t) + 0.5 * t) + 0.6 * torch.randn(N, generator=g)
    return dict(X=X, y=y)


def subset(X, M, seed):
    """The rows GPHead.fit(inducing_points=M, seed=seed) draws."""
    return X[torch.randperm(X.shape[0], generator=torch.Generator().manual_seed(int(seed)))[:M]].clone()


def sqdist(X, Z):
    return torch.cdist(X.to(torch.float64), Z.to(torch.float64), compute_mode="donot_use_mm_for_euclid_dist") ** 2


def kernel_centroid(Z):
    """mean_m z_m in fp64, rounded to fp32 as the kernel's operand is; returned in fp64."""
    return Z.to(torch.float64).mean(dim=0).to(torch.float32).to(torch.float64)


def lowest_argmin(d):
    """Per row the lowest index among the exact minima of d [N, M]."""
    M = d.shape[1]
    index = torch.arange(M).expand_as(d)
    return torch.where(d == d.min(dim=1, keepdim=True).values, index, torch.full_like(index, M)).min(dim=1).values


def sums_of(X, Z, assign, centroid=None):
    """(counts [M], wss [M], sums [M, D]) of an assignment, fp64; `centroid` defaults to kernel_centroid(Z)."""
    M = Z.shape[0]
    a = assign.to(torch.int64)
    cen = kernel_centroid(Z) if centroid is None else centroid.to(torch.float64)
    d = sqdist(X, Z)
    counts = torch.bincount(a, minlength=M).to(torch.float64)
    wss = torch.zeros(M, dtype=torch.float64).index_add_(0, a, d[torch.arange(X.shape[0]), a])
    sums = torch.zeros(M, Z.shape[1], dtype=torch.float64).index_add_(0, a, X.to(torch.float64) - cen)
    return counts, wss, sums


def step(X, Z):
    """One restated step: dict(assign, counts, wss, sums, centroid, d2 [N, M], bound [N], gap [N])."""
    d = sqdist(X, Z)
    assign = lowest_argmin(d)
    counts, wss, sums = sums_of(X, Z, assign)
    Z64 = Z.to(torch.float64)
    cbar = Z64.mean(dim=0)
    D = Z.shape[1]
    bound = 8.0 * (D + 3) * 2.0 ** -24 * (((X.to(torch.float64) - cbar) ** 2).sum(1) + ((Z64 - cbar) ** 2).sum(1).max())
    if Z.shape[0] > 1:
        two = torch.topk(d, 2, dim=1, largest=False).values
        gap = two[:, 1] - two[:, 0]
    else:
        gap = torch.full((X.shape[0],), math.inf, dtype=torch.float64)
    return dict(assign=assign, counts=counts, wss=wss, sums=sums, centroid=kernel_centroid(Z), d2=d, bound=bound, gap=gap)


def update(Z, st):
    """The centres after the step `st` taken at Z: fp32."""
    filled = st["counts"] > 0
    moved = st["centroid"] + st["sums"] / st["counts"].clamp_min(1.0)[:, None]
    return torch.where(filled[:, None], moved, Z.to(torch.float64)).to(torch.float32)


def lloyd(X, Z0, iters):
    """The restated loop from Z0 (fp32): dict(Z: the centres each step started from and, last, the returned ones;
    steps: the step dicts; iterations, converged, inertia, empty as the package reports them)."""
    Z, Zs, steps = Z0.to(torch.float32), [Z0.to(torch.float32)], []
    rep = dict(iterations=0, converged=False, inertia=[], empty=[])
    for _ in range(iters):
        st = step(X, Z)
        rep["inertia"].append(float(st["wss"].sum()))
        if steps and torch.equal(st["assign"], steps[-1]["assign"]):
            steps.append(st)
            rep["converged"] = True
            break
        steps.append(st)
        Z = update(Z, st)
        Zs.append(Z)
        rep["empty"].append(int((st["counts"] == 0).sum()))
        rep["iterations"] += 1
    return dict(Z=Zs, steps=steps, **rep)


def first_of_equal(Z):
    """Per centre the lowest index of a centre with the same bits."""
    same = (Z[:, None, :] == Z[None, :, :]).all(-1)
    return lowest_argmin((~same).to(torch.float64))


def assignment_figures(got, st, Z, scale=1.0):
    """How an assignment `got` [N] meets the near-tie rule at the restated step `st`, with the bound scaled by `scale`:
    dict(wrong_clear: rows with gap > scale B that did not receive the restatement's centre, excess: the largest fp64
    distance of a received centre above the row's minimum over scale B_n (<= 1 passes), not_lowest: rows that received
    a centre with a bit-identical one below it, near: rows with gap <= scale B)."""
    a = got.to(torch.int64)
    rows = torch.arange(a.shape[0])
    B = scale * st["bound"]
    clear = st["gap"] > B
    over = st["d2"][rows, a] - st["d2"].min(dim=1).values
    return dict(wrong_clear=int((clear & (a != st["assign"])).sum()), excess=float((over / B).max()),
                not_lowest=int((first_of_equal(Z)[a] != a).sum()), near=int((~clear).sum()))


def eager_fp32_step(X, Z, chunk=4096):
    """What an eager fp32 evaluation gives, centred as the kernel centres: (assign, counts, wss, sums); the distances as
    |xc|^2 + |zc|^2 - 2 xc zc^T, argmin, index_add_ in fp32 per chunk of rows, the chunks added in fp64."""
    f32 = torch.float32
    cen = kernel_centroid(Z)
    Zc = (Z.to(torch.float64) - cen).to(f32)
    zn = (Zc * Zc).sum(1)
    M, D = Z.shape
    assign = torch.empty(X.shape[0], dtype=torch.int64)
    counts, wss, sums = (torch.zeros(M, dtype=torch.float64), torch.zeros(M, dtype=torch.float64),
                         torch.zeros(M, D, dtype=torch.float64))
    for i in range(0, X.shape[0], chunk):
        xc = X[i:i + chunk].to(f32) - cen.to(f32)
        d = ((xc * xc).sum(1, keepdim=True) + zn[None, :] - 2.0 * (xc @ Zc.T)).clamp_min(0)
        best, a = d.min(dim=1)
        assign[i:i + chunk] = a
        counts += torch.bincount(a, minlength=M).to(torch.float64)
        wss += torch.zeros(M, dtype=f32).index_add_(0, a, best).to(torch.float64)
        sums += torch.zeros(M, D, dtype=f32).index_add_(0, a, xc).to(torch.float64)
    return assign, counts, wss, sums


def sum_errors(got_wss, got_sums, ref_wss, ref_sums):
    """{name: (error, bound)}, bound = 1e-4 of the quantity's max-norm in the restatement."""
    return {"wss": (float((got_wss - ref_wss).abs().max()), PARITY * float(ref_wss.abs().max())),
            "sums": (float((got_sums - ref_sums).abs().max()), PARITY * float(ref_sums.abs().max()))}


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and the restated step of a step case; computed once, shared, never modified."""
    kw = CASES[name]
    inp = build_inputs(**kw)
    return dict(inp=inp, step=step(inp["X"], inp["Z"]), N=kw["N"], M=kw["M"], D=kw["D"], chunk_rows=kw.get("chunk_rows"),
                ldx_pad=kw.get("ldx_pad", 0))


@functools.lru_cache(maxsize=None)
def lloyd_case(name):
    """Inputs, the subset start and the restated loop of a Lloyd fixture; computed once, shared, never modified."""
    kw = LLOYD_CASES[name]
    inp = build_lloyd_inputs(**kw)
    Z0 = subset(inp["X"], kw["M"], kw["seed"])
    return dict(inp=inp, Z0=Z0, ref=lloyd(inp["X"], Z0, LLOYD_ITERS), N=kw["N"], M=kw["M"], D=kw["D"], seed=kw["seed"],
                chunk_rows=kw.get("chunk_rows"))


SPECIAL = ("centroid_rows", "duplicates", "far_centre")


@functools.lru_cache(maxsize=None)
def special(name):
    """Step inputs built from the cases for one hazard each: dict(X, Z, step, chunk_rows, ldx_pad, marked).
    centroid_rows: 40 rows at the fp32 centroid of the 33 centres of n150_m33_d5 and 27 rows within 1e-3 of it, where a
                   padded centre (Mp = 64: zero image, zero norm) would be at distance ~0;
    duplicates:    n300_m96_d65 with three centres overwritten by a copy of the lowest centre that has rows (`marked`:
                   [that centre, the copies]);
    far_centre:    the start of the Lloyd fixture n150_m6_d5 with centre 3 moved by +50 in every column (`marked`: 3)."""
    if name == "centroid_rows":
        Z = case("n150_m33_d5")["inp"]["Z"]
        cen = kernel_centroid(Z).to(torch.float32)
        g = torch.Generator().manual_seed(11)
        X = torch.cat([cen.expand(40, -1), cen + 1e-3 * torch.randn(27, Z.shape[1], generator=g)]).contiguous()
        extra = dict(chunk_rows=32, ldx_pad=0, marked=None)
    elif name == "duplicates":
        c = case("n300_m96_d65")
        X, Z = c["inp"]["X"], c["inp"]["Z"].clone()
        first = int((c["step"]["counts"] > 0).nonzero()[0])
        copies = sorted({m for m in (first + 1, 64, 95) if m > first})
        Z[copies] = Z[first].clone()
        extra = dict(chunk_rows=None, ldx_pad=3, marked=[first, copies])
    else:
        c = lloyd_case("n150_m6_d5")
        X, Z = c["inp"]["X"], c["Z0"].clone()
        Z[3] = Z[3] + 50.0
        extra = dict(chunk_rows=64, ldx_pad=0, marked=3)
    return dict(X=X, Z=Z, step=step(X, Z), **extra)


def restated_elbo(X, y, Z, s, ell):
    """The collapsed bound of gp_fit_cases at Z, the targets normalised by the training rows as GPHead.fit does."""
    y_norm, _, _ = gp_fit_cases.normalise(y)
    return gp_fit_cases.solve(gp_fit_cases.statistics(X, y_norm, Z, s, ell), X.shape[0], s)["elbo"]
