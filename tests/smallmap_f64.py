"""float64 reference of the interpolator for the small-map schedule tests, with RESOLVED LeakyReLU masks (no GPU needed to import).

The forward output of the interpolator is continuous in every pre-activation, so a kernel's output goes against float64 directly.  The
gradients are not: a pre-activation within rounding of zero may take either side of its LeakyReLU in a correct fp32 kernel, and one such
flip moves a gradient tensor by ~1e-3 (tests/test_gpu_modules.py::test_interpolator_default_gradient_deviation_not_above_torch_fp32).
Instead of hoping that no element is near zero, the reference here finds out which side the implementation under test took:

  recording forward   generator_forward() re-states oracle.afigan_oracle.generator_forward op by op (bit-identical in float64), records every
                      LeakyReLU pre-activation tensor and forces the mask of chosen (tensor, flat index) elements to the opposite side.
  candidate set S     elements with |z| < GUARD * sqrt(K) * eps * max|z| of their tensor; K = taps x input channels of the conv that made
                      z, eps = 2^-24, GUARD = 4 = twice the per-conv C_MAX that tests/test_gpu_pixgemm.py measured and enforces.  |S| <= CAP
                      is a condition on the reference alone (a case that exceeds it gets another seed).
  flip effect         delta_e = grads(reference with e flipped) - grads(reference), one float64 forward + backward per candidate.
  resolution          r = got - ref over all gradient tensors, each divided by its own ||ref||; c_e = <r, delta_e> / <delta_e, delta_e>,
                      taken over all candidates at once (the least-squares c of r ~ sum_e c_e delta_e: the same number when the deltas
                      are orthogonal, and they are not quite -- in case b the flip of one head-conv element alone projects 0.117 onto the
                      delta of a conv-transpose element downstream of it, which the one-by-one quotient would call unresolvable).
                      |c_e| <= 0.1: not flipped; |c_e - 1| <= 0.1: flipped; anything else: unresolvable (AssertionError).  A candidate whose
                      delta is below the comparison bar in every tensor counts as not flipped.
  final comparison    the reference once more with exactly the resolved flips; the implementation is compared with that.

A flip OUTSIDE S means a forward error above the guard: nothing explains it away, it stays in the comparison as a deviation of ~1e-3.

Bars (eps = 2^-24; max-norm relative to max|ref| of the tensor, and the relative L2, both against the same number):
  forward output                    C_F * sqrt(9 * (C + 4G)) * eps
  dx and every parameter gradient   C_G * sqrt(max(9 * (C + 4G), 4 * N * H * W)) * eps
C_F and C_G: twice the worst ratio measured over the case table of tests/test_gpu_smallmap.py, rounded up (its docstring has the figures).

wk6_tile_forms() mirrors the rule by which the launchers of csrc/smallmap.hip choose between the 32x32 and the 32x64 tile of the bf16x6
small-map kernel; the profiler cannot tell the two apart (both record as kind 20).
"""
import math

import torch
import torch.nn.functional as F

from oracle import afigan_oracle as orc

EPS = 2.0 ** -24
GUARD = 4.0            # candidate threshold: GUARD * sqrt(K) * eps * max|z| (twice C_MAX of tests/test_gpu_pixgemm.py)
CAP = 64               # |S| <= CAP for every case, asserted on the reference alone
C_F = 1.0              # forward bar: C_F * sqrt(9 (C + 4G)) * eps (measured: <= 0.05)
C_G = 2.0              # gradient bar: C_G * sqrt(max(9 (C + 4G), 4 N H W)) * eps (measured: <= 0.95)
MAX_BAR = 1e-4         # no max-norm bar of a case may exceed this (ten times under the whole-call tests' 1e-3)


# ------------------------------------------------------------------------------------------------ recording forward
def act_names(n_rdb):
    """the LeakyReLU pre-activation tensors of one interpolator call, in forward order"""
    return ["a0"] + [f"rdb{r}.conv{k}" for r in range(n_rdb) for k in range(1, 5)] + ["a7", "u"]


def act_K(name, C, G):
    """reduction length (taps x input channels) of the conv that produces pre-activation tensor `name`; the conv-transpose k6 s2 p2
    reads 3 x 3 input pixels per output pixel (conv_transpose_6s2p2_phases)"""
    if name.startswith("rdb"):
        k = int(name[-1])
        return 9 * (C + (k - 1) * G)
    return 9 * C


def generator_forward(x, p, n_rdb=3, residual_scale=0.2, flips=None, record=None):
    """oracle.afigan_oracle.generator_forward, op by op.  record: a dict that receives {act_names() entry: detached pre-activation};
    flips: {act_names() entry: [flat indices]} whose LeakyReLU mask is forced to the opposite side (value AND gradient follow the mask)."""
    flips = flips or {}

    def lrelu(z, name):
        if record is not None:
            record[name] = z.detach()
        m = z > 0
        idx = flips.get(name)
        if idx is not None and len(idx):
            idx = torch.as_tensor(sorted(idx), dtype=torch.int64, device=z.device)
            mv = m.reshape(-1)
            assert mv.data_ptr() == m.data_ptr()
            mv[idx] = ~mv[idx]
        return torch.where(m, z, z * orc.LRELU_SLOPE)

    a0 = lrelu(F.conv2d(x, p["Generators.0.0.0.weight"], p["Generators.0.0.0.bias"], 1, 1), "a0")
    h = a0
    for r in range(n_rdb):
        prefix = f"Generators.0.1.RDBs.{r}"
        feats = [h]
        for k in range(1, 5):
            c = F.conv2d(torch.cat(feats, 1), p[f"{prefix}.conv{k}.0.weight"], None, 1, 1)
            feats.append(lrelu(c, f"rdb{r}.conv{k}"))
        c5 = F.conv2d(torch.cat(feats, 1), p[f"{prefix}.conv5.weight"], None, 1, 1)
        h = h + c5 * residual_scale
    t = h * residual_scale + a0
    a7 = lrelu(F.conv2d(t, p["Generators.0.2.0.weight"], p["Generators.0.2.0.bias"], 1, 1), "a7")
    u = lrelu(orc.conv_transpose_6s2p2_phases(a7, p["Generators.0.3.0.weight"], p["Generators.0.3.0.bias"]), "u")
    g = F.conv2d(u, p["Generators.0.4.0.weight"], p["Generators.0.4.0.bias"], 1, 1)
    return g + orc.bilinear2x(x)


def run(x, p, Rw, n_rdb, flips=None, record=None, want_dx=True, dtype=torch.float64, device=None):
    """forward + backward of the loss (out * Rw).sum() in `dtype` on `device`: (out, {"dx": .., parameter name: gradient}) as float64"""
    device = device or x.device
    pp = {k: v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k, v in p.items()}
    xx = x.detach().to(device=device, dtype=dtype).clone().requires_grad_(want_dx)
    out = generator_forward(xx, pp, n_rdb, flips=flips, record=record)
    (out * Rw.to(device=device, dtype=dtype)).sum().backward()
    grads = {k: v.grad.double() for k, v in pp.items()}
    if want_dx:
        grads["dx"] = xx.grad.double()
    return out.detach().double(), grads


def candidates(record, C, G):
    """S: [(tensor name, flat index)] with |z| < GUARD * sqrt(K) * eps * max|z| of the tensor, in forward order"""
    S = []
    for name, z in record.items():
        thr = GUARD * math.sqrt(act_K(name, C, G)) * EPS * z.abs().max().item()
        for i in torch.nonzero(z.reshape(-1).abs() < thr).flatten().tolist():
            S.append((name, i))
    return S


# ------------------------------------------------------------------------------------------------ bars
def bar_fwd(C, G):
    return C_F * math.sqrt(9 * (C + 4 * G)) * EPS


def bar_grad(C, G, N, H, W):
    return C_G * math.sqrt(max(9 * (C + 4 * G), 4 * N * H * W)) * EPS


def errs(got, ref):
    """(max|got - ref| / max|ref|, ||got - ref|| / ||ref||)"""
    d = (got.double() - ref.double()).flatten()
    r = ref.double().flatten()
    return (d.abs().max() / r.abs().max().clamp_min(1e-300)).item(), (d.norm() / r.norm().clamp_min(1e-300)).item()


# ------------------------------------------------------------------------------------------------ reference with resolved masks
def _flipdict(elems):
    d = {}
    for name, i in elems:
        d.setdefault(name, []).append(i)
    return d


class Reference:
    """The float64 reference of one case: output, gradients, candidate set, flip effects (computed on `device`, on first use)."""

    def __init__(self, x, p, Rw, C, G, n_rdb, want_dx=True, device="cpu"):
        self.x, self.p, self.Rw, self.C, self.G, self.n_rdb, self.want_dx, self.device = x, p, Rw, C, G, n_rdb, want_dx, device
        self.N, _, self.H, self.W = x.shape
        rec = {}
        self.out, self.grads = self._run(None, rec)
        self.S = candidates(rec, C, G)
        self.n_act = sum(z.numel() for z in rec.values())
        assert len(self.S) <= CAP, f"|S| = {len(self.S)} > {CAP}: the reference has too many near-zero pre-activations, change the case's seed"
        self.bar_f = bar_fwd(C, G)
        self.bar_g = bar_grad(C, G, self.N, self.H, self.W)
        assert self.bar_f <= MAX_BAR and self.bar_g <= MAX_BAR, (self.bar_f, self.bar_g)
        self._deltas = None

    def _run(self, elems, record=None):
        return run(self.x, self.p, self.Rw, self.n_rdb, flips=_flipdict(elems) if elems else None, record=record, want_dx=self.want_dx,
                   device=self.device)

    def deltas(self):
        if self._deltas is None:
            self._deltas = []
            for e in self.S:
                g = self._run([e])[1]
                self._deltas.append({k: g[k] - self.grads[k] for k in g})
        return self._deltas

    def _vec(self, g, keys):
        return torch.cat([(g[k].to(self.grads[k].device) / self.grads[k].norm().clamp_min(1e-300)).flatten() for k in keys])

    def resolve(self, got):
        """got: {name: gradient} (a subset of the reference's tensors).  Returns the elements of S whose mask the implementation took on the
        other side; AssertionError when a candidate's coefficient is neither 0 nor 1 within 0.1."""
        keys = [k for k in self.grads if k in got]
        assert keys and set(got) <= set(self.grads), sorted(set(got) - set(self.grads))
        r = self._vec({k: got[k].double().to(self.grads[k].device) - self.grads[k] for k in keys}, keys)
        live, cols = [], []
        for e, d in zip(self.S, self.deltas()):
            if all((d[k].abs().max() / self.grads[k].abs().max().clamp_min(1e-300)).item() < self.bar_g for k in keys):
                continue                                    # its effect is below the bar everywhere: not flipped
            live.append(e)
            cols.append(self._vec(d, keys))
        if not live:
            return []
        D = torch.stack(cols)                               # [candidates, gradient elements]
        gram, b = D @ D.T, D @ r
        c = torch.linalg.solve(gram, b)                     # (diagonal Gram matrix: c_e = <r, delta_e> / <delta_e, delta_e>)
        flipped = []
        for e, ce in zip(live, c.tolist()):
            if abs(ce - 1.0) <= 0.1:
                flipped.append(e)
            else:
                assert abs(ce) <= 0.1, f"candidate {e}: coefficient {ce:.3f} is neither 0 nor 1: the deviation is not a mask flip"
        return flipped

    def resolved(self, got):
        """(gradients of the reference evaluated with exactly the flips `got` took, those flips)"""
        flipped = self.resolve(got)
        return (self._run(flipped)[1] if flipped else self.grads), flipped

    def check_grads(self, got, tag="", report=print):
        """resolve, then hold every tensor of `got` to the gradient bar (max-norm and relative L2); returns (flips, worst error / bar)"""
        ref, flipped = self.resolved(got)
        worst, lines = 0.0, []
        for k in got:
            em, el = errs(got[k].to(ref[k].device), ref[k])
            worst = max(worst, em / self.bar_g, el / self.bar_g)
            lines.append((k, em, el))
        k, em, el = max(lines, key=lambda t: max(t[1], t[2]))
        report(f"[smallmap] {tag} |S| {len(self.S)} of {self.n_act} activations, flips {len(flipped)} {flipped}; worst gradient {k}: "
               f"max-norm {em:.2e} rel-L2 {el:.2e} (bar {self.bar_g:.2e}, {worst * C_G:.2f} sqrt(K) eps)")
        for k, em, el in lines:
            assert em <= self.bar_g, f"{tag} {k}: max-norm rel error {em:.3e} > bar {self.bar_g:.3e} (|S| {len(self.S)}, flips {flipped})"
            assert el <= self.bar_g, f"{tag} {k}: rel-L2 error {el:.3e} > bar {self.bar_g:.3e} (|S| {len(self.S)}, flips {flipped})"
        return flipped, worst

    def check_out(self, out, tag="", cpu32=None, report=print):
        em, el = errs(out.to(self.out.device), self.out)
        extra = ""
        if cpu32 is not None:
            cm, cl = errs(cpu32.to(self.out.device), self.out)
            extra = f"; torch cpu fp32: max-norm {cm:.2e} rel-L2 {cl:.2e}"
        worst = max(em, el) / self.bar_f
        report(f"[smallmap] {tag} forward: max-norm {em:.2e} rel-L2 {el:.2e} (bar {self.bar_f:.2e}, {worst * C_F:.2f} sqrt(K) eps){extra}")
        assert em <= self.bar_f, f"{tag} out: max-norm rel error {em:.3e} > bar {self.bar_f:.3e}"
        assert el <= self.bar_f, f"{tag} out: rel-L2 error {el:.3e} > bar {self.bar_f:.3e}"
        return worst


# ------------------------------------------------------------------------------------------------ the 32x64 tile rule, mirrored
def _cdiv(a, b):
    return -(-a // b)


def _wide_candidate(ncols, nK):
    """wk6_wide_candidate (csrc/smallmap.hip)"""
    return ncols >= 64 and nK >= 16


def _single_wide(M, ncols, Ck, nKphase=1):
    """launch_wk: one problem on an image takes the 32x64 kernel when it is a candidate and still has >= 128 tiles that way"""
    nK = 9 * nKphase * _cdiv(Ck, 32)
    return _wide_candidate(ncols, nK) and _cdiv(M, 32) * _cdiv(ncols, 64) >= 128


def _group_wide(M, probs):
    """afi_launch_pix_gemm_wk_group: probs = [(Ncols, Ck)]; the group takes the 32x64 kernel when a problem is a candidate and the launch
    still has >= 128 tiles with the candidates widened"""
    ntm, tiles, any_wide = _cdiv(M, 32), 0, False
    for ncols, Ck in probs:
        cand = _wide_candidate(ncols, 9 * _cdiv(Ck, 32))
        any_wide = any_wide or cand
        tiles += ntm * _cdiv(ncols, 64 if cand else 32)
    return any_wide and tiles >= 128


def wk6_tile_forms(C, G, R, N, H, W, want_dx=True):
    """Which launches of a forward + backward ON WEIGHT IMAGES (default arithmetic, C % 32 == G % 32 == 0, P <= 4096) take the 32x64 form of
    the bf16x6 small-map kernel: {"single_wide": [...], "single_narrow": [...], "group_wide": [...], "group_narrow": [...]} of launch names.
    This MIRRORS wk6_wide_candidate and the `>= 128 tiles` rules of launch_wk / afi_launch_pix_gemm_wk_group as gen_plan()'s schedule calls
    them; it does not observe a launch."""
    P, L = N * H * W, C + 4 * G
    hires = 4 * P <= 4096
    out = {"single_wide": [], "single_narrow": [], "group_wide": [], "group_narrow": []}

    def single(name, M, ncols, Ck, nKphase=1):
        out["single_wide" if _single_wide(M, ncols, Ck, nKphase) else "single_narrow"].append(name)

    single("head", P, C, C)
    for r in range(R):
        for j in range(5):
            nch = C if j == 0 else G
            probs = [(G, nch) for _k in range(j + 1, 5)] + [(C, nch)]
            out["group_wide" if _group_wide(P, probs) else "group_narrow"].append(f"rdb{r}.step{j}")
    single("trunk", P, C, C)
    single("convT", P, 4 * C, C)
    if hires:
        single("final", 4 * P, C, C)
        single("final.dgrad", 4 * P, C, C)
    single("convT.dgrad", P, C, C, 4)
    single("trunk.dgrad", P, C, C)
    for r in range(R):
        single(f"rdb{r}.conv5.dgrad", P, L, C)
        for k in range(1, 5):
            single(f"rdb{r}.conv{k}.dgrad", P, C + (k - 1) * G, G)
    if want_dx:
        single("head.dgrad", P, C, C)
    return out
