"""Any-length transforms on the GPU (pf.any_length_descriptor: stockham_wg_bluestein_kernel): every transform of every
case against NumPy in double precision -- forward np.fft.fft, backward N * np.fft.ifft -- with the project's two
yardsticks unchanged (per-transform relative L2 within helpers.REL_L2_TOL, helpers.check_reference_rule with n = N),
through gpu_utils.transform_packed: guard bands, the unchanged input of an out-of-place execute and the write set
(padded distances, offsets, in place, a base pointer one element off 128-byte alignment).

The lengths all have a prime factor above 61 and are refused without the extension bit.  Beside the lengths of the
issue (which all land on the convolution lengths P = 256, 2048, 4096, 8192), 251 and 509 cover P = 512 and 1024.

Measured on the MI355X (worst transform of every case of a length, forward and backward):
fp32 rel-L2 1.5e-7 ... 3.2e-7, fp64 3.5e-16 ... 6.7e-16.

No case is skipped: a commit that answers unsupported_configuration inside the supported set fails the test."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

LENGTHS = {"f32": [67, 127, 251, 509, 67 * 8, 521, 1021, 1031, 2039, 2 * 2039, 4093, 4094],
           "f64": [67, 127, 251, 509, 67 * 8, 1021, 1031, 2039, 2047]}
CASES = [(p, n) for p in ("f32", "f64") for n in LENGTHS[p]]
# one batch of several thousand groups (many trips of the persistent loop) per kernel configuration
BIG = {("f32", 127), ("f32", 251), ("f32", 509), ("f32", 1021), ("f32", 2039), ("f32", 4093),
       ("f64", 127), ("f64", 251), ("f64", 509), ("f64", 1021), ("f64", 2039)}


def _mods():
    import gpu_utils as G
    import portfft_amd as pf
    return G, pf, G.torch_mod()


def _ct(prec):
    return np.complex64 if prec == "f32" else np.complex128


def _conv_length(n):
    p = 1
    while p < 2 * n - 1:
        p *= 2
    return p


def _desc(pf, n, prec, batch=1, in_place=False, distances=None, offsets=(0, 0), scales=(1.0, 1.0)):
    d = pf.any_length_descriptor([n], prec)
    d.number_of_transforms = batch
    d.forward_scale, d.backward_scale = scales
    d.forward_offset, d.backward_offset = offsets
    if distances is not None:
        d.forward_distance, d.backward_distance = distances
    if in_place:
        d.placement = pf.placement.IN_PLACE
    return d


def _data(rng, batch, n, ct):
    return (rng.uniform(-1, 1, (batch, n)) + 1j * rng.uniform(-1, 1, (batch, n))).astype(ct)


def _check(got, ref, ct, n, what):
    got = np.asarray(got).astype(np.complex128)
    ref = np.asarray(ref).astype(np.complex128)
    err = np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)
    print("%s: worst rel-L2 %.3e (transform %d)" % (what, float(err.max()), int(np.argmax(err))))
    assert np.all(err <= H.REL_L2_TOL[np.dtype(ct)]), (what, "transform", int(np.argmax(err)), float(err.max()))
    assert H.check_reference_rule(got, ref.astype(ct), n), (what, "per-element reference rule")


def _both_directions(G, pf, d, x, what, guard=None):
    """forward and backward of the packed rows x through d's layout, every transform checked"""
    ct, n = x.dtype.type, x.shape[1]
    guard = G.GUARD if guard is None else guard
    plan = d.commit()
    y, _ = G.transform_packed(d, pf.direction.FORWARD, x, plan, guard)
    _check(y, d.forward_scale * np.fft.fft(x.astype(np.complex128), axis=1), ct, n, what + ("fwd",))
    z, _ = G.transform_packed(d, pf.direction.BACKWARD, x, plan, guard)
    _check(z, d.backward_scale * n * np.fft.ifft(x.astype(np.complex128), axis=1), ct, n, what + ("bwd",))


@pytest.mark.parametrize("prec,n", CASES)
def test_any_length_transforms_against_numpy(prec, n):
    G, pf, torch = _mods()
    ct = _ct(prec)
    info = _desc(pf, n, prec).commit().info()
    dim = info.dims[0]
    assert dim.length == n and dim.tier == 1 and tuple(info.launches) == (1, 1)
    assert int(np.prod(dim.factors[:dim.n_factors])) == _conv_length(n) != n
    assert dim.lds_bytes > 0
    print("N=%d %s: P=%d factors %s fpw %d lds %d" % (n, prec, _conv_length(n), list(dim.factors[:dim.n_factors]),
                                                     dim.ffts_per_workgroup, dim.lds_bytes))
    fpw = max(1, dim.ffts_per_workgroup)
    rng = np.random.Generator(np.random.SFC64(n))
    batches = sorted({1, 3, 2 * fpw - 1, 2 * fpw + 1} | ({4000 * fpw + 1} if (prec, n) in BIG else set()))
    for batch in batches:
        x = _data(rng, batch, n, ct)
        _both_directions(G, pf, _desc(pf, n, prec, batch), x, (prec, n, batch, "oop"))
        _both_directions(G, pf, _desc(pf, n, prec, batch, in_place=True), x, (prec, n, batch, "ip"))
        if batch in (3, 2 * fpw + 1):
            scales = (0.5, 0.25 / n)
            # padded rows on one side, packed rows on the other, different offsets; base one element off 128 bytes
            _both_directions(G, pf, _desc(pf, n, prec, batch, False, (n + 5, n), (5, 2), scales), x,
                             (prec, n, batch, "oop padded input"), guard=(65, 63))
            _both_directions(G, pf, _desc(pf, n, prec, batch, False, (n, n + 5), (0, 3), scales), x,
                             (prec, n, batch, "oop padded output"))
            _both_directions(G, pf, _desc(pf, n, prec, batch, True, (n + 5, n + 5), (3, 3), scales), x,
                             (prec, n, batch, "ip padded"), guard=(63, 65))


@pytest.mark.parametrize("prec,n", [("f32", 127), ("f32", 1031), ("f32", 4093), ("f64", 1021), ("f64", 2039)])
def test_round_trip_clone_and_events(prec, n):
    G, pf, torch = _mods()
    ct = _ct(prec)
    batch = 5
    x = _data(np.random.Generator(np.random.SFC64(7 * n)), batch, n, ct)
    d = _desc(pf, n, prec, batch)
    plan = d.commit()
    y, ybits = G.transform_packed(d, pf.direction.FORWARD, x, plan)
    back, _ = G.transform_packed(d, pf.direction.BACKWARD, y.astype(ct), plan)
    _check(back, n * x.astype(np.complex128), ct, n, (prec, n, "round trip"))
    # a cloned plan on a second stream gives the same bits
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        clone = plan.copy()
        _, cbits = G.transform_packed(d, pf.direction.FORWARD, x, clone)
    H.check_unchanged(ybits, cbits, what="cloned plan")
    # an execute ordered by `dependencies`: the returned event's completion means valid data
    seen = {}

    class with_events:
        wait = staticmethod(plan.wait)

        @staticmethod
        def compute_forward(*bufs):
            dep = torch.cuda.Event()
            dep.record(torch.cuda.current_stream())
            ev = plan.compute_forward(*bufs, dependencies=[dep])
            assert ev.native
            ev.wait()
            assert ev.is_complete()
            seen["bits"] = bufs[-1].cpu().numpy().copy()  # read right behind the event, before any other wait

    _, ebits = G.transform_packed(d, pf.direction.FORWARD, x, with_events)
    H.check_unchanged(ybits, ebits, what="execute with a dependency and a returned event")
    H.check_unchanged(ybits, seen["bits"][:ybits.size], what="the output behind the returned event")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_smooth_length_with_the_bit_is_the_plain_plan(prec):
    G, pf, torch = _mods()
    ct = _ct(prec)
    n, batch = 1000, 7
    x = _data(np.random.Generator(np.random.SFC64(1000)), batch, n, ct)
    plain = G.make_descriptor([n], prec, batch=batch)
    withbit = _desc(pf, n, prec, batch)
    pi, wi = plain.commit().info(), withbit.commit().info()
    assert tuple(pi.dims[0].factors[:pi.dims[0].n_factors]) == tuple(wi.dims[0].factors[:wi.dims[0].n_factors])
    assert pi.dims[0].tier == wi.dims[0].tier and int(np.prod(wi.dims[0].factors[:wi.dims[0].n_factors])) == n
    for direction in (pf.direction.FORWARD, pf.direction.BACKWARD):
        _, a = G.transform_packed(plain, direction, x)
        _, b = G.transform_packed(withbit, direction, x)
        H.check_unchanged(a, b, what="length 1000 with PFFT_EXT_ANY_LENGTH")


def test_refusals_name_the_cause():
    G, pf, torch = _mods()
    for prec, lengths, reason in (("f32", [4099], "its convolution length P"), ("f32", [67 * 64], "its convolution length P"),
                                  ("f64", [2053], "its convolution length P"), ("f32", [127, 4], "1-D")):
        with pytest.raises(pf.unsupported_configuration) as e:
            pf.any_length_descriptor(lengths, prec).commit()
        assert reason in str(e.value), (lengths, str(e.value))
        if "convolution" in reason:
            assert "has no LDS-resident plan" in str(e.value)
    with pytest.raises(pf.unsupported_configuration):
        pf.descriptor([127], "f32").commit()  # without the bit: the reference's answer
    with pytest.raises(pf.unsupported_configuration):
        pf.any_length_descriptor([4093], "f16").commit()
