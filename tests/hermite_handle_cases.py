"""The refusals the three Hermite handles answer alike, through the raw C ABI (tests/test_hermite_gpu.py,
test_hermite_block_gpu.py, test_hermite_batch_gpu.py run raw_refusals once each): null state arrays, a particle count
above the capacity, the state precision read back and, for the two block-step handles, the three parameter checks."""
import ctypes as C

import numpy as np


def raw_refusals(nb, ctx, d, family, owner, layout=None):
    """family: "" (nbody_hip_hermite_*), "block_" or "batch_"; owner: the word of the capacity message; layout: the
    offsets of an ensemble.  d: the particle data on the device."""
    lib = nb._lib.load()
    fn = lambda tail: getattr(lib, f"nbody_hip_hermite_{family}{tail}")  # noqa: E731
    OK, VALIDATION = nb._lib.OK, nb._lib.ERR_VALIDATION
    n = d.count
    s = d.struct()
    systems = () if layout is None else (len(layout) - 1,)
    rng = np.random.default_rng(3)
    pos, vel = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    got_pos, got_vel = np.empty((n, 3)), np.empty((n, 3))

    # a particle count above the capacity
    small = C.c_void_p()
    nb._lib.check(fn("create")(ctx.handle, n - 1, *systems, C.byref(small)))
    for call, a, b in ((fn("set_state_f64"), pos, vel), (fn("get_state_f64"), got_pos, got_vel)):
        assert call(small, C.byref(s), a.ctypes.data, b.ctypes.data) == VALIDATION
        assert lib.nbody_hip_last_error().startswith(
            f"particle count {n} exceeds the {owner} capacity {n - 1}".encode()), lib.nbody_hip_last_error()
    assert fn("destroy")(small) == OK

    h = C.c_void_p()
    nb._lib.check(fn("create")(ctx.handle, n, *systems, C.byref(h)))
    try:
        if layout is not None:
            off = np.asarray(layout, np.uint64)
            nb._lib.check(fn("set_layout")(h, off.ctypes.data, off.size - 1))
        # null state arrays
        for call in (fn("set_state_f64"), fn("get_state_f64")):
            for a, b in ((None, got_vel.ctypes.data), (got_pos.ctypes.data, None)):
                assert call(h, C.byref(s), a, b) == VALIDATION
                assert lib.nbody_hip_last_error().startswith(b"null state array"), lib.nbody_hip_last_error()
        # the state precision comes back as it was set
        mode = C.c_int(-1)
        assert fn("get_precision")(h, C.byref(mode)) == OK and mode.value == 0
        assert fn("set_precision")(h, 1) == OK
        assert fn("get_precision")(h, C.byref(mode)) == OK and mode.value == 1
        # the three parameter checks, each with its message
        if family:
            for args, what in (((0.0, 0.01, 16), b"eta must be positive and finite"),
                               ((0.02, float("inf"), 16), b"eta_start must be positive and finite"),
                               ((0.02, 0.01, 21), b"max_level must be in [0, 20], got 21")):
                assert fn("set_params")(h, *args) == VALIDATION, args
                assert lib.nbody_hip_last_error().startswith(what), lib.nbody_hip_last_error()
            assert fn("set_params")(h, 0.02, 0.01, 20) == OK
        # none of the refusals left the handle unusable: the extended state goes in and comes back as hi + lo
        assert fn("set_state_f64")(h, C.byref(s), pos.ctypes.data, vel.ctypes.data) == OK
        assert fn("get_state_f64")(h, C.byref(s), got_pos.ctypes.data, got_vel.ctypes.data) == OK
        for got, want in ((got_pos, pos), (got_vel, vel)):
            assert np.all(np.abs(got - want) <= 2.0 ** -48 * np.abs(want))
    finally:
        assert fn("destroy")(h) == OK
