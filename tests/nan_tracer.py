"""The NaN tracer: one NaN planted in one input of a training kernel marks exactly the outputs that depend on that element.

The criterion of tests/test_gpu_nan_tracer.py has no tolerance.  With ``got_clean`` the kernel's result without the plant,
``got_planted`` its result with it and ``ref_planted`` the float64 definition (tests/*_f64.py, on the CPU) of the planted input:

  * isnan(got_planted) == isnan(ref_planted) at every element -- a NaN goes where torch sends it and only there;
  * everywhere else got_planted has the BITS of got_clean (compared as int32).

One refinement, decided by the definition alone: an output that is not NaN may still depend on the planted element through a discrete
decision that a NaN decides one way -- a ReLU gate that a NaN leaves open (torch's backward closes on `<= 0` only), sign(NaN) = 0, the
pooling route that goes to a window's last NaN.  There the float64 definition's value moves from ``ref_clean`` to another value that is NOT the result of arithmetic on the
plant: an exact 0 or an exact copy of a float32 input.  ``expected`` takes that value from the definition, asserts that float32 holds it
exactly, and compares it by value (a gate closed by a select gives +0 and one closed by a product -0).  A sum that gains or loses finite
terms this way is a third kind: with stored statistics the case table avoids it by construction (``open_at``: the planted elements have
open gates in the clean input already); with batch statistics a NaN channel opens every gate of the channel, so its bias gradient becomes
the plain sum of the arriving gradient, and the fused LeakyReLU of the 4x4 convolution turns the gate of a NaN output into the slope --
those cases name the outputs this can happen to (``Case.rederived``: the bias gradient; dx, dw, db of the leaky convolution), and
tests/test_nan_tracer_host.py asserts from the definitions that it happens to no other output of any case.

Plants (``plants``): element (0, 0) of plane (0, 0); an interior element; the last element of the last plane; an element of the last
channel (of a ragged channel count where the case has one); the first element of sample 1, which catches reads across samples.  One
plant per run, NaN only (inf * 0 would muddle the map).

The case table (``CASES``) holds, per case, the seeded inputs, the names of the inputs that are planted and the float64 definition of
every output; the device side of each case lives in tests/test_gpu_nan_tracer.py.  A case that expected "everything NaN" or "nothing
NaN" would prove little: tests/test_nan_tracer_host.py asserts over the whole table that weights and incoming gradients hold no exact
zero and that every (case, input, plant) has an output with 0 < count(isnan(ref)) < numel, the reductions named in ``ALL_OR_NOTHING``
excepted.

Definitions that had to change for a NaN to go where torch sends it (the finite values are the same):
  * block_train_f64.bn_train_grads / decoder_train_f64.bn_nz_train_grads formed the gated gradient as a product ga * [y > 0]; torch's
    ReLU backward SELECTS and closes on `<= 0` only, so a NaN arriving at a closed gate stops there and a NaN pre-activation passes the
    gradient on -- which is how train_step_f64's autograd sends a NaN into the batch-norm bias of a NaN channel.  They do the same now.
  * block_train_f64.resample / resample_adjoint multiply by a matrix that is mostly exact zeros, which spreads a NaN over its whole row
    and column; here the resampling stages are torch's own avg_pool2d / interpolate and their float64 autograd, the yardstick
    tests/test_gpu_block_train.py already uses for them.
Test infrastructure only."""
import functools

import torch
import torch.nn.functional as F

import adam_f64 as A64
import block_train_f64 as B64
import conv_train_f64 as C64
import decoder_train_f64 as G64
import disc_f64 as D64
import spectral_f64 as S64

NAN = float("nan")


# ------------------------------------------------------------------ the criterion

def expected(got_clean, ref_planted, ref_clean=None, rederived=False):
    """(expected, by_value, free): ``got_clean`` with NaN written wherever the float64 definition of the planted input is NaN and, given
    the definition of the clean input too, with the definition's value wherever that moved to another number that float32 holds exactly
    (``by_value`` marks those elements).  ``rederived``: the case says that finite results are formed again from a decision the plant
    changed (the LeakyReLU gate of a NaN output is the slope, so the weight gradient loses (1 - slope) of finite terms); such elements
    are ``free``: they have no clean-run bits to keep, must not be NaN, and tests/test_gpu_nan_tracer.py holds them to float64 with the
    criterion of tests/test_gpu_disc.py (E_gpu <= 10 E_plain32 + 1e-6).  Without it a moved value that float32 does not hold is an
    error of the case."""
    got_clean, ref_planted = torch.as_tensor(got_clean), torch.as_tensor(ref_planted)
    assert got_clean.dtype == torch.float32 and tuple(got_clean.shape) == tuple(ref_planted.shape), (got_clean.dtype, got_clean.shape, ref_planted.shape)
    nan = torch.isnan(ref_planted)
    out = torch.where(nan, torch.full_like(got_clean, NAN), got_clean)
    moved, free = torch.zeros_like(nan), torch.zeros_like(nan)
    if ref_clean is not None:
        moved = ~nan & (ref_planted != torch.as_tensor(ref_clean))
        value = ref_planted.to(torch.float32)
        free = moved & (value.to(ref_planted.dtype) != ref_planted)
        assert rederived or not bool(free.any()), "a moved value that float32 does not hold: arithmetic on the plant"
        moved = moved & ~free
        out = torch.where(moved, value, out)
    return out, moved, free


def mismatches(got_planted, got_clean, ref_planted, ref_clean=None, rederived=False):
    """(elements whose NaN-ness differs from the definition's, elements that are NaN in neither but differ from the clean run)."""
    want, by_value, free = expected(got_clean, ref_planted, ref_clean, rederived)
    got = torch.as_tensor(got_planted)
    assert got.dtype == torch.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    same_bits = got.contiguous().view(torch.int32) == want.contiguous().view(torch.int32)
    same = torch.where(by_value, got == want, same_bits) | free
    return int((nan_g != nan_w).sum()), int((~same & ~nan_g & ~nan_w).sum())


def check(name, got_planted, got_clean, ref_planted, ref_clean=None):
    footprint, bits = mismatches(got_planted, got_clean, ref_planted, ref_clean)
    n_ref, n_got = int(torch.isnan(torch.as_tensor(ref_planted)).sum()), int(torch.isnan(torch.as_tensor(got_planted)).sum())
    assert footprint == 0 and bits == 0, (f"{name}: {footprint} elements differ in NaN-ness from float64 (float64 has {n_ref} NaN, the kernel "
                                          f"{n_got}), {bits} elements outside the footprint lost the bits of the clean run")


# ------------------------------------------------------------------ the plants

def plants(shape, ragged=None):
    """{name: index} for a tensor of ``shape`` (4-D: [N,C,H,W] or [Cout,Cin,k,k]; 2-D and 1-D tensors get what exists of it)."""
    if len(shape) == 4:
        a, b, h, w = shape
        out = {"origin": (0, 0, 0, 0), "interior": (0, b // 2, h // 2, w // 2), "last": (a - 1, b - 1, h - 1, w - 1),
               "last_channel": (0, b - 1, h // 2, (w - 1) // 3)}
        if a > 1:
            out["sample1"] = (1, 0, 0, 0)
        return out
    if len(shape) == 2:
        a, b = shape
        return {"origin": (0, 0), "interior": (a // 2, b // 2), "last": (a - 1, b - 1)}
    n, = shape
    return {"origin": (0,), "interior": (n // 2,), "last": (n - 1,)}


def planted(t, index):
    """A copy of ``t`` with NaN at ``index`` (or at every index of a list: the windows with two NaNs)."""
    out = t.clone()
    for i in (index if isinstance(index, list) else [index]):
        out[tuple(i)] = NAN
    return out


def assert_dense(t, name=""):
    assert bool(torch.isfinite(t).all()) and bool((t != 0).all()), f"{name}: dense finite values without an exact zero required"


def open_at(x, scale, shift, where):
    """x with the elements at the indices ``where`` moved so that the float64 pre-activation x * scale - shift is +1 there: their ReLU
    gates are open in the clean run, as torch's ReLU backward (closed on `<= 0` only) leaves them for a NaN (scale, shift [N,C] float64)."""
    x = x.clone()
    for n, c, i, j in where:
        x[n, c, i, j] = float((shift[n, c] + 1.0) / scale[n, c])
        assert float(x[n, c, i, j].double() * scale[n, c] - shift[n, c]) > 0.5
    return x


# ------------------------------------------------------------------ the case table

class Case:
    """name; make() -> {input name: float32 CPU tensor or setting}; ref(inputs in float64) -> {output name: tensor}; plant: the inputs
    that get the plants; dense: the inputs asserted to hold no zero; extra: {input name: {plant name: index or list of indices}}."""

    def __init__(self, name, make, ref, plant, dense=(), extra=None, ragged=False, only=None, rederived=()):
        self.name, self._make, self._ref, self.plant, self.dense, self.extra, self.ragged = name, make, ref, tuple(plant), tuple(dense), extra or {}, ragged
        self.rederived = tuple(rederived)                # the outputs that may hold re-derived elements (see ``expected``); no other may
        self.only = only or {}                           # {input name: function(case) -> its plants}, instead of the standard ones

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        return self._make()

    def plants(self, key):
        if key in self.only:
            return self.only[key](self)
        out = plants(tuple(self.inputs()[key].shape))
        out.update(self.extra.get(key, {}))
        return out

    def with_plant(self, key, index):
        return dict(self.inputs(), **{key: planted(self.inputs()[key], index)})

    def ref(self, inputs=None, dtype=torch.float64):
        """The float64 definition of ``inputs`` (default: the clean ones); dtype=torch.float32: the same definition in float32 on the CPU,
        which sizes the bound of the re-derived elements."""
        inputs = self.inputs() if inputs is None else inputs
        with torch.no_grad():
            out = self._ref({k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inputs.items()})
        return {k: v.detach() for k, v in out.items() if v is not None}

    @functools.lru_cache(maxsize=None)
    def ref_clean(self):
        return self.ref()

    def runs(self):
        return [(key, pname, index) for key in self.plant for pname, index in self.plants(key).items()]


CASES = {}
# (case, planted input[, plant]) whose every output is all-NaN or all-clean BY DEFINITION: a scalar loss that is NaN while its gradient
# holds no NaN (sign(NaN) = 0); an element no pooling window holds.  Everything else must show a
# partial footprint in some output.
ALL_OR_NOTHING = set()


def _add(case, all_or_nothing=()):
    assert case.name not in CASES, case.name
    CASES[case.name] = case
    ALL_OR_NOTHING.update((case.name,) + (key if isinstance(key, tuple) else (key,)) for key in all_or_nothing)
    return case


_sid = lambda s: "x".join(map(str, s))                                    # noqa: E731


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(v) * 7 ** i for i, v in enumerate(seed)) + 17)


# ---- 1. the 3x3 convolutions (fp32 rung): one tile; ragged tiles (Cin 40, Cout 72, 660 pixels); more than one pixel chunk per slab
CONV3_SHAPES = ((2, 3, 32, 16, 16), (2, 40, 72, 33, 20), (2, 8, 8, 5, 7))
SPLITS = (0, 1, 3)


def _conv_inputs(shape, k, out_hw=None):
    N, cin, cout, H, W = shape
    gen = _gen(cin, cout, H, k)
    r = lambda *s: torch.randn(*s, generator=gen)                          # noqa: E731
    OH, OW = out_hw or (H, W)
    return dict(x=r(N, cin, H, W), w=r(cout, cin, k, k) / (k * cin ** 0.5), b=r(cout), g=r(N, cout, OH, OW) * (1.0 + torch.arange(OW) / OW))


def _conv3_ref(i):
    return dict(out=C64.conv(i["x"], i["w"], i["b"]), dx=C64.conv_dx(i["g"], i["w"]), dw=C64.conv_dw(i["x"], i["g"]), db=C64.conv_db(i["g"]))


def _pconv_inputs(shape):
    i = _conv_inputs(shape, 3)
    i["mask"] = C64.holed_mask(shape[0], shape[3], shape[4], seed=shape[1] + shape[3])
    return i


def _pconv_ref(i):
    """partial_conv3x3(x * mask, mask, w, b): the definition's x * mask decides what a NaN in the mask plane touches."""
    xm = i["x"] * i["mask"]
    out, um = C64.pconv(xm, i["mask"], i["w"], i["b"])
    dx, dw, db = C64.pconv_grads(xm, i["mask"], i["w"], i["g"])
    return dict(out=out, um=um, dx=dx, dw=dw, db=db)


for _s in CONV3_SHAPES:
    _add(Case("conv3x3-" + _sid(_s), functools.partial(_conv_inputs, _s, 3), _conv3_ref, ("x", "w", "g"), ("x", "w", "g"), ragged=_s[1] % 32 != 0))
for _s in CONV3_SHAPES[1:]:
    _add(Case("pconv3x3-" + _sid(_s), functools.partial(_pconv_inputs, _s), _pconv_ref, ("x", "mask", "w", "g"), ("x", "w", "g")))


# ---- slr_conv_grad_scale_bias: Gr = G r, db = sum G um
SCALE_BIAS_SHAPES = ((2, 40, 33, 20), (2, 8, 5, 7), (2, 64, 37, 51))


def _scale_bias_inputs(shape):
    N, C, H, W = shape
    _, um, r = C64.partial_factors(C64.holed_mask(N, H, W, seed=C), 16)
    return dict(g=torch.randn(N, C, H, W, generator=_gen(C, H)), r=r, um=um)


for _s in SCALE_BIAS_SHAPES:
    _add(Case("scale_bias-" + _sid(_s), functools.partial(_scale_bias_inputs, _s),
              lambda i: dict(gr=i["g"] * i["r"], db=C64.conv_db(i["g"] * i["um"])), ("g", "r"), ("g",)))


# ---- 2. the 1x1 convolution and its weight gradient
CONV1_SHAPES = ((2, 3, 32, 16, 16), (2, 40, 72, 33, 20), (2, 64, 64, 5, 7))

for _s in CONV1_SHAPES:
    _add(Case("conv1x1-" + _sid(_s), functools.partial(_conv_inputs, _s, 1),
              lambda i: dict(out=B64.conv1x1(i["x"], i["w"], i["b"]), dx=B64.conv1x1_dx(i["g"], i["w"]), dw=B64.conv1x1_dw(i["x"], i["g"]),
                             db=C64.conv_db(i["g"])), ("x", "w", "g"), ("x", "w", "g"), ragged=_s[1] % 32 != 0))


# ---- 3. the 4x4 convolution: stride 1 and 2, with and without the fused LeakyReLU (its gate reaches the backward), odd sizes (all four
# parity classes of the stride-2 backward), ragged channels, the K split (two and more summed channels)
CONV4_SHAPES = ((2, 3, 64, 33, 20, 2), (2, 40, 72, 33, 20, 1), (2, 8, 8, 5, 7, 2))


def _conv4_inputs(shape, leaky):
    N, cin, cout, H, W, s = shape
    i = _conv_inputs(shape[:5], 4, (D64.out_size(H, s), D64.out_size(W, s)))
    i.update(stride=s, leaky=leaky)
    return i


def conv4_backward_data(g, w, s, H, W):
    """disc_f64.conv_backward_data over a gradient zero-padded by two pixels: the same numbers, and every definition here treats a NaN
    WEIGHT the same way.  conv_train_f64.conv / conv_dx and disc_f64.conv_forward gather over a zero-padded operand, so a border pixel's
    absent terms are 0 x w = NaN for a NaN weight; disc_f64.conv_backward_data scatters and has no such terms (in a stride-2 parity
    class: 170 instead of 160 pixels per plane at 33 x 20).  The kernels are gather-form GEMMs over a zero-padded operand like the
    former.  A NaN weight is NaN in every pixel that any tap of its parity reaches; nothing in x or g is affected by the choice."""
    gp = F.pad(g, (2, 2, 2, 2))
    OH, OW = gp.shape[2:]
    full = g.new_zeros(g.shape[0], w.shape[1], s * (OH - 1) + 4, s * (OW - 1) + 4)
    for ky in range(4):
        for kx in range(4):
            full[:, :, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s] += torch.einsum("nohw,oc->nchw", gp, w[:, :, ky, kx])
    o = 2 + 2 * s
    assert o + H <= full.shape[2] and o + W <= full.shape[3]
    return full[:, :, o:o + H, o:o + W].contiguous()


def _conv4_ref(i):
    s, (H, W) = i["stride"], i["x"].shape[2:]
    raw = D64.conv_forward(i["x"], i["w"], i["b"], s)
    g = i["g"] * D64.leaky_gate(raw) if i["leaky"] else i["g"]
    dw, db = D64.conv_weight_grad(i["x"], g, s)
    return dict(out=D64.leaky(raw) if i["leaky"] else raw, dx=conv4_backward_data(g, i["w"], s, H, W), dw=dw, db=db)


for _s in CONV4_SHAPES:
    for _l in (False, True):
        _add(Case(f"conv4x4-{_sid(_s)}-{'leaky' if _l else 'plain'}", functools.partial(_conv4_inputs, _s, _l), _conv4_ref, ("x", "w", "g"),
                  ("x", "w", "g"), ragged=_s[1] % 32 != 0, rederived=("dx", "dw", "db") if _l else ()))


# ---- Conv4x4s2 of the motion encoder (slr_conv4x4s2_forward: stride 2, padding 1, LeakyReLU of the value read, bias, then the affine
# epilogue y * scale[c] + shift[c]); forward only -- the motion networks do not learn here.  The body is conv4x4_kernel's, the padding,
# the LeakyReLU in front and the per-channel epilogue are its own: odd and even sizes, ragged channels, with and without each.
CONV4S2_SHAPES = ((2, 40, 72, 33, 20, True, True), (2, 3, 64, 16, 20, False, True), (2, 8, 8, 5, 7, True, False))      # ..., leaky, affine


def _conv4s2_inputs(shape):
    N, cin, cout, H, W, leaky, affine = shape
    i = _conv_inputs((N, cin, cout, H, W), 4)
    del i["g"]
    gen = _gen(cin, cout, W)
    i.update(leaky=leaky)
    if affine:
        i.update(scale=1.0 + 0.3 * torch.randn(cout, generator=gen), shift=torch.randn(cout, generator=gen))
    return i


def _conv4s2_ref(i):
    x = D64.leaky(i["x"]) if i["leaky"] else i["x"]
    H, W = x.shape[2:]
    OH, OW = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_zeros(x.shape[0], i["w"].shape[0], OH, OW)
    for ky in range(4):
        for kx in range(4):
            out += torch.einsum("nchw,oc->nohw", xp[:, :, ky:ky + 2 * (OH - 1) + 1:2, kx:kx + 2 * (OW - 1) + 1:2], i["w"][:, :, ky, kx])
    out = out + i["b"].view(1, -1, 1, 1)
    if "scale" in i:
        out = out * i["scale"].view(1, -1, 1, 1) + i["shift"].view(1, -1, 1, 1)
    return dict(out=out)


for _s in CONV4S2_SHAPES:
    _add(Case("conv4x4s2-" + _sid(_s[:5]), functools.partial(_conv4s2_inputs, _s), _conv4s2_ref,
              ("x", "w", "b") + (("scale", "shift") if _s[6] else ()), ("x", "w", "b") + (("scale", "shift") if _s[6] else ()), ragged=_s[1] % 32 != 0))


# ---- 4. the batch-norm family: 5 x 7 (the scalar body) and 16 x 20 (the 16-byte body); C = 24 runs in both layouts, C = 5 is ragged
BN_SHAPES = ((2, 24, 5, 7), (2, 24, 16, 20), (2, 5, 5, 7))


def _bn_inputs(shape, masked, stored, nonzero=False):
    N, C, H, W = shape
    mask = C64.holed_mask(N, H, W, seed=C + W) if masked else None
    x, gain, bias, ga = B64.bn_inputs(N, C, H, W, seed=C * 10 + H, mask=mask)
    gen = _gen(C, H, int(stored))
    if nonzero:
        x = x * G64.keep_pattern(N, C, H, W, seed=C + H, zero_channel=False)
    out = dict(x=x, gain=gain, bias=bias, ga=ga)
    if masked:
        out["mask"] = mask
    if stored:
        out["mean"], out["var"] = torch.randn(C, generator=gen), 0.3 + 2 * torch.rand(C, generator=gen)
        scale, shift = B64.bn_tables(out["mean"].double(), out["var"].double(), gain.double(), bias.double())
        out["x"] = open_at(x, scale, shift, plants(shape).values())
    return out


def _open_gate_plants(pre):
    """The plants of the gradient arriving at a gated activation: a NaN at a closed gate stops there (torch's ReLU backward selects), so
    each standard plant moves to the open gate nearest to it in its own plane.  pre(inputs in float64) -> the open gates [N,C,H,W]."""
    def of(case):
        inp = case.inputs()
        with torch.no_grad():
            gate = pre({k: (v.double() if torch.is_tensor(v) else v) for k, v in inp.items()})
        W, out = gate.shape[3], {}
        for name, (n, c, i, j) in plants(tuple(gate.shape)).items():
            while not bool(gate[n, c].any()):            # (a plane of closed gates: the next channel of the same sample)
                c = (c + 1) % gate.shape[1]
            flat = gate[n, c].reshape(-1).nonzero().reshape(-1)
            at = int(flat[(flat - (i * W + j)).abs().argmin()])
            out[name] = (n, c, at // W, at % W)
        return out
    return of


def _bn_gates(i, nonzero=False):
    if "mean" in i:
        mean, var = i["mean"], i["var"]
    else:
        mean, var = (G64.bn_nz_stats(i["x"]) if nonzero else B64.bn_stats(i["x"], i.get("mask")))[:2]
    scale, shift = B64.bn_tables(mean, var, i["gain"], i["bias"])
    open_ = (i["x"] * B64._t(scale) - B64._t(shift)) > 0
    if nonzero:
        open_ = open_ & (i["x"] != 0)
    return open_ if i.get("mask") is None else open_ & (i["mask"] > 0)


def _bn_ref(i):
    st = (i["mean"], i["var"]) if "mean" in i else None
    a, mean, var = B64.bn_train(i["x"], i.get("mask"), i["gain"], i["bias"], stored=st)
    dx, dgain, dbias = B64.bn_train_grads(i["x"], i.get("mask"), i["gain"], i["bias"], i["ga"], stored=st)
    out = dict(a=a, dx=dx, dgain=dgain, dbias=dbias)
    if st is None:
        out.update(mean=mean, var=var)
    return out


def _bn_nz_ref(i):
    st = (i["mean"], i["var"]) if "mean" in i else None
    a, mean, var, msum = G64.bn_nz_train(i["x"], i["gain"], i["bias"], stored=st)
    dx, dgain, dbias = G64.bn_nz_train_grads(i["x"], i["gain"], i["bias"], i["ga"], stored=st)
    out = dict(a=a, msum=msum, dx=dx, dgain=dgain, dbias=dbias)
    if st is None:
        out.update(mean=mean, var=var)
    return out


for _s in BN_SHAPES:
    for _stored in (False, True):
        for _masked in (False, True):
            _add(Case(f"bn-{_sid(_s)}-{'mask' if _masked else 'nomask'}-{'stored' if _stored else 'batch'}",
                      functools.partial(_bn_inputs, _s, _masked, _stored), _bn_ref, ("x", "ga"), ("ga", "gain"), ragged=_s[1] % 8 != 0,
                      only={"ga": _open_gate_plants(_bn_gates)}, rederived=() if _stored else ("dbias",)))
        _add(Case(f"bn_nonzero-{_sid(_s)}-{'stored' if _stored else 'batch'}", functools.partial(_bn_inputs, _s, False, _stored, True),
                  _bn_nz_ref, ("x", "ga"), ("ga", "gain"), ragged=_s[1] % 8 != 0, only={"ga": _open_gate_plants(functools.partial(_bn_gates, nonzero=True))},
                  rederived=() if _stored else ("dbias",)))


# ---- slr_pconv_train_epilogue: out = (raw * ratio + bias) * um (+ residual)
def _epilogue_inputs(shape):
    N, C, H, W = shape
    gen = _gen(C, W)
    msum = (torch.rand(N, 1, H, W, generator=gen) * 4).floor()
    msum[:, :, :2, :4] = 0.0
    ratio, um, _ = G64.partial_factors_counts(msum, C)
    assert bool((um == 0).any()) and bool((um == 1).any())
    return dict(raw=torch.randn(N, C, H, W, generator=gen), ratio=ratio, um=um, bias=torch.randn(C, generator=gen), residual=torch.randn(N, C, H, W, generator=gen))


for _s in BN_SHAPES:
    _add(Case("pconv_epilogue-" + _sid(_s), functools.partial(_epilogue_inputs, _s),
              lambda i: dict(out=(i["raw"] * i["ratio"] + i["bias"].view(1, -1, 1, 1)) * i["um"] + i["residual"]), ("raw", "residual", "ratio"),
              ("raw", "residual", "bias"), ragged=_s[1] % 8 != 0))


# ---- 5. the resampling stages and their adjoints, odd and even sizes (the plants' "last" is on the last row and column)
RESAMPLE = tuple((kind, hw) for kind in ("Down", "Up") for hw in ((5, 7), (16, 20)))


def _resample_fn(kind):
    return (lambda t: F.avg_pool2d(t, 3, stride=2, padding=1)) if kind == "Down" else \
        (lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False))


def _resample_inputs(kind, hw):
    gen = _gen(*hw)
    x = torch.randn(2, 8, *hw, generator=gen)
    return dict(x=x, g=torch.randn(_resample_fn(kind)(x).shape, generator=gen), kind=kind)


def _resample_ref(i):
    with torch.enable_grad():
        x = i["x"].clone().requires_grad_(True)
        y = _resample_fn(i["kind"])(x)
        dx, = torch.autograd.grad(y, x, i["g"])
    return dict(y=y, dx=dx)


for _k, _hw in RESAMPLE:
    _add(Case(f"resample-{_k}-{_sid(_hw)}", functools.partial(_resample_inputs, _k, _hw), _resample_ref, ("x", "g"), ("x", "g")))


# ---- 6. instance norm + LeakyReLU: a plant touches its plane only
NORM_SHAPES = ((2, 5, 5, 7), (2, 8, 16, 20))

for _s in NORM_SHAPES:
    _add(Case("instnorm-" + _sid(_s), functools.partial(lambda s: dict(x=D64.nudged(torch.randn(*s, generator=_gen(*s))),
                                                                         gy=torch.randn(*s, generator=_gen(*s, 1))), _s),
              lambda i: (lambda y, xh, rstd: dict(y=y, dx=D64.instnorm_lrelu_backward(i["gy"], xh, rstd)))(*D64.instnorm_lrelu_forward(i["x"])),
              ("x", "gy"), ("x", "gy"), ragged=_s[1] % 8 != 0))


# ---- 7. the loss kernels
L1_SHAPES = ((2, 3, 5, 7), (2, 3, 16, 20))
L1_SCALE = 3.0                                           # the gradient arriving at the loss


def _l1_ref(i):
    d = i["pred"] - i["gt"]
    # (1 / n and the arriving gradient are float32 numbers multiplied in float32 by the kernel: the product is formed that way here,
    #  so that the definition's gradient is a value float32 holds)
    k = (torch.tensor(1.0 / d.numel(), dtype=torch.float32) * torch.tensor(L1_SCALE, dtype=torch.float32)).double()
    return dict(loss=d.abs().mean().reshape(1), grad=torch.sign(d) * k)


for _s in L1_SHAPES:
    _add(Case("l1-" + _sid(_s), functools.partial(lambda s: dict(pred=torch.rand(*s, generator=_gen(*s)), gt=torch.rand(*s, generator=_gen(*s, 2))), _s),
              _l1_ref, ("pred", "gt"), (), ), all_or_nothing=("pred", "gt"))

GATE_SHAPES = ((2, 8, 5, 7), (2, 24, 16, 20))
GATE_MODES = ("seed", "seed+g_in", "relu")
GATE_COEF, GATE_SCALE = 0.37, 1.7


def _gate_inputs(shape, mode):
    gen = _gen(*shape)
    a = torch.randn(*shape, generator=gen)
    return dict(a=a, b=a + 0.5 * torch.randn(*shape, generator=gen), g=torch.randn(*shape, generator=gen), mode=mode)


def _gate_ref(i):
    a, mode = i["a"], i["mode"]
    g = i["g"] if mode != "seed" else torch.zeros_like(a)
    if mode == "relu":
        return dict(out=torch.where(a <= 0, torch.zeros_like(g), g))
    d = torch.relu(a) - torch.relu(i["b"])
    k = (torch.tensor(GATE_COEF / a.numel(), dtype=torch.float32) * torch.tensor(GATE_SCALE, dtype=torch.float32)).double()
    return dict(out=torch.where(a <= 0, torch.zeros_like(g), g + torch.sign(d) * k), sum=d.abs().sum().reshape(1))


for _s in GATE_SHAPES:
    for _m in GATE_MODES:
        _planted = {"seed": ("a", "b"), "seed+g_in": ("a", "b", "g"), "relu": ("a", "g")}[_m]
        # a NaN in a or b: the sum is NaN and the gradient holds none (sign(NaN) = 0, and the gate torch closes on `<= 0` only passes
        # g itself); in g it goes through open gates only
        _add(Case(f"gate-{_sid(_s)}-{_m}", functools.partial(_gate_inputs, _s, _m), _gate_ref, _planted, ("g",),
                  only={"g": _open_gate_plants(lambda i: i["a"] > 0)}), all_or_nothing=[k for k in _planted if k != "g"])

POOL_SHAPES = ((2, 8, 5, 7), (2, 16, 8, 12))


def _pool_ref(i):
    with torch.enable_grad():
        x = i["x"].clone().requires_grad_(True)
        y = F.max_pool2d(torch.relu(x), 2, 2)
        dx, = torch.autograd.grad(y, x, i["g"])
    return dict(y=y, dx=dx)


def _pool_inputs(shape):
    N, C, H, W = shape
    gen = _gen(*shape)
    return dict(x=torch.randn(*shape, generator=gen), g=torch.randn(N, C, H // 2, W // 2, generator=gen))


for _s in POOL_SHAPES:
    # windows with two NaNs: torch's max_pool2d routes the gradient to the LAST one in row-major order
    _two = {"two_in_a_row": [(0, 1, 2, 2), (0, 1, 2, 3)], "two_on_the_diagonal": [(1, 3, 0, 0), (1, 3, 1, 1)], "all_four": [(0, 2, 0, 2), (0, 2, 0, 3), (0, 2, 1, 2), (0, 2, 1, 3)]}
    # the gradient of a window goes on only if the window's maximum is positive: its plants move to the nearest such window
    _add(Case("relu_maxpool-" + _sid(_s), functools.partial(_pool_inputs, _s), _pool_ref, ("x", "g"), ("x", "g"), extra={"x": _two},
              only={"g": _open_gate_plants(lambda i: F.max_pool2d(i["x"], 2, 2) > 0)}),
         all_or_nothing=[("x", "last")] if _s[2] % 2 else ())    # (floor mode: the last row and column of an odd size are not pooled)


# ---- 8. the multi-tensor operators
ADAM_SETTING, ADAM_K = 3, 1                              # the resumed state: m, v and the step count set; one step


def _adam_inputs():
    """The tensor list of tests/test_gpu_adam.py (adam_f64.case: 15 tensors, every size class of the kernel, three of them misaligned
    views -- that file has no list of 130; the 130 misaligned tensors are the spectral case's) as flat inputs; the device side cuts
    them back into the list."""
    ts = A64.case(ADAM_SETTING)
    cat = lambda key: torch.cat([t[key] for t in ts])                      # noqa: E731
    return dict(p=cat("p0"), m=cat("m0"), v=cat("v0"), g=torch.cat([t["grads"][0] for t in ts]))


def adam_cuts():
    return [t["p0"].numel() for t in A64.case(ADAM_SETTING)]


def _adam_ref(i):
    beta1, beta2, lr, _, t0 = A64.SETTINGS[ADAM_SETTING]
    p, m, v, _ = A64.run(i["p"], [i["g"]], i["m"], i["v"], t0, lr, beta1, beta2)
    return dict(p=p, m=m, v=v)


def _adam_plants():
    cuts, out, at = adam_cuts(), {}, 0
    for j, n in enumerate(cuts):
        if n in (1, 5, 65) or j >= len(cuts) - 3:        # a one-element tensor, a scalar tail, past a wavefront, the three misaligned views
            out[f"tensor{j}_of_{n}"] = (at + n // 2,)
            out[f"tensor{j}_last"] = (at + n - 1,)
        at += n
    return out


_add(Case("adam", _adam_inputs, _adam_ref, ("g",), (), only={"g": lambda case: _adam_plants()}))

SPECTRAL_N = 130


def _spectral_inputs():
    from test_spectral_f64 import SIGMA_SHAPES
    out = {"shapes": tuple(SIGMA_SHAPES[i % len(SIGMA_SHAPES)] for i in range(SPECTRAL_N))}
    ws, us, vs, dws = [], [], [], []
    for i, (r, c) in enumerate(out["shapes"]):
        W, u, v = S64.matrix_case(r, c, 100 + i)
        ws.append(W.float().reshape(-1)), us.append(u.float()), vs.append(v.float())
        dws.append(torch.randn(r * c, generator=_gen(i, r, c)))
    out.update(w=torch.cat(ws), u=torch.cat(us), v=torch.cat(vs), dw=torch.cat(dws))
    return out


def spectral_split(flat, shapes, what):
    """The flat input cut back into the list: what = "w" ([r, c] matrices), "u" ([r]) or "v" ([c])."""
    sizes = [r * c if what == "w" else r if what == "u" else c for r, c in shapes]
    parts = torch.split(flat, sizes)
    return [p.view(r, c) for p, (r, c) in zip(parts, shapes)] if what == "w" else list(parts)


def _spectral_ref(i):
    """One training power iteration per tensor, 1 / sigma, and the gradient to weight_orig for the gradient dw at the effective weight."""
    shapes = i["shapes"]
    inv, us, vs, grads = [], [], [], []
    for W, u, v, dW in zip(spectral_split(i["w"], shapes, "w"), spectral_split(i["u"], shapes, "u"), spectral_split(i["v"], shapes, "v"),
                           spectral_split(i["dw"], shapes, "w")):
        _, u1, v1, inv_sigma = S64.effective(W, u, v, True)
        inv.append(inv_sigma.reshape(1)), us.append(u1), vs.append(v1)
        grads.append(S64.weight_orig_grad(dW, W, u1, v1, inv_sigma).reshape(-1))
    return dict(inv_sigma=torch.cat(inv), u=torch.cat(us), v=torch.cat(vs), grad=torch.cat(grads))


def _spectral_plants():
    from test_spectral_f64 import SIGMA_SHAPES
    shapes = [SIGMA_SHAPES[i % len(SIGMA_SHAPES)] for i in range(SPECTRAL_N)]
    starts = [0]
    for r, c in shapes:
        starts.append(starts[-1] + r * c)
    out = {}
    for j in (0, 1, len(SIGMA_SHAPES) + 2, SPECTRAL_N - 1):
        r, c = shapes[j]
        out[f"tensor{j}_first"] = (starts[j],)
        out[f"tensor{j}_interior"] = (starts[j] + (r // 2) * c + c // 2,)
        out[f"tensor{j}_last"] = (starts[j + 1] - 1,)
    return out


# (the flat tensors' own origin / interior / last say nothing more than the lists' plants)
_add(Case("spectral", _spectral_inputs, _spectral_ref, ("w",), (), only={"w": lambda case: _spectral_plants()}))


# ------------------------------------------------------------------ what the host test asserts over the table

def footprint_counts(case, key, index):
    """{output: (NaN count of the float64 definition, numel)} for one plant."""
    ref = case.ref(case.with_plant(key, index))
    return {k: (int(torch.isnan(v).sum()), v.numel()) for k, v in ref.items()}


def partial_somewhere(counts):
    return any(0 < n < numel for n, numel in counts.values())



# ---- 9. one whole iteration, the generator step only (train_step_f64.iteration_gradients at the fixture shape, batch 2 at 32 x 32)
ITERATION_PLANTS = {"pixel": ("images", (0, 1, 2, 17, 9)),               # one pixel of the start image of sample 1
                    "decoder_weight": ("sd/projector.eblocks.3.conv_aa.weight_orig", (1, 2, 1, 1))}


def iteration_case(plant=None):
    """(fixture, inputs) of tests/train_step_f64.py with the named plant (None: clean): the fixture dict holds the initial state."""
    import train_step_f64 as T
    g = T.load()
    inputs = T.fixture_inputs(g)
    if plant is not None:
        key, index = ITERATION_PLANTS[plant]
        if key == "images":
            images = [t.clone() for t in inputs["images"]]
            images[index[0]][tuple(index[1:])] = NAN
            inputs = dict(inputs, images=images)
        else:
            a = g[key].copy()
            a[tuple(index)] = NAN
            g = dict(g, **{key: a})
    return g, inputs


def iteration_ref(g, inputs):
    """({loss entry: float64 scalar}, {reference key: the parameter after the generator's optimiser step}) of the float64 iteration
    without the discriminator: the gradients of train_step_f64.iteration_gradients, then adam_f64.step from a fresh state with the
    trainer's settings (lr_g, betas (0.99, beta2) without a discriminator)."""
    import train_step_f64 as T
    opts = T.options(discriminator_losses="0")
    r = T.iteration_gradients([inputs], None, torch.float64, False, opts=opts, g=g)
    leaves = T.generator(g, torch.float64)["leaves"]
    after = {}
    for k, grad in r["grads_G"].items():
        p = leaves[k].detach()
        after[k] = A64.step(p, grad, torch.zeros_like(p), torch.zeros_like(p), 1, opts.lr_g, 0.99, opts.beta2)[0]
    return {k: v.reshape(()) for k, v in r["losses"].items()}, after
