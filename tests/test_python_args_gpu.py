"""What the Python binding does with its tensor arguments, for every Plan method that takes device tensors: one table, ROWS, of
(method, model, tensor arguments, call).  A later method is covered by adding its row; test_every_method_has_a_row says when one is missing.

Every row is held to three things, at B = 3 on the smallest models that reach the method -- the three-link chain with rotors for the
explicit calls, tello_with_arms (a floating base and implicit clusters) for state conversion, projection and the contact calls:
  strided inputs   every input given as a view big[::2] gives the bits of the call on contiguous tensors; a tensor the call writes in
                   place (project_positions' q, a caller's out) is refused when it has strides
  one exception rule  a CPU tensor or an int64 tensor: GrbdaError(-3), "no CPU fallback"; one float32 among float64: TypeError; a row
                   short by one column: ValueError -- raised before anything is enqueued
  a side stream    the call on stream=side with strided inputs gives the bits of the call on the current stream
The last shows that the call runs on the stream it was given; that every tensor is recorded on that stream is read off the one helper
(Plan._call and its companions), not tested here."""
import functools
import inspect

import numpy as np
import pytest

import generalized_rbda_amd as G
import entry_points as EP
from generalized_rbda_amd import modeldesc as md

pytestmark = pytest.mark.gpu
B, T, DT = 3, 2, 1e-3


@functools.lru_cache(maxsize=None)
def _blob(model):
    return md.revolute_chain_with_rotor(3).serialize() if model == "chain" else EP._model(model)


@functools.lru_cache(maxsize=None)
def _host_inputs(model):
    """the numpy inputs of a model, float64; shared, never written to"""
    blob = _blob(model)
    plan = G.Plan(blob)
    q, qd, tau = EP._states(blob, B, 5)
    rng = np.random.default_rng(17)
    return {"q": q, "qd": qd, "tau": tau, "fext": rng.uniform(-1, 1, (B, plan.n_bodies, 6)), "force": rng.uniform(-1, 1, (B, 3)),
            "a_des": rng.uniform(-1, 1, (B, 1, 3)), "tau_T": tau[None] * rng.uniform(0.4, 1.0, (T, B, 1)),
            "q_start": q + rng.uniform(-0.02, 0.02, q.shape), "out": np.zeros_like(tau), "q_next": np.zeros_like(q)}


def _contiguous(v, gpu):
    import torch

    return torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=gpu)


def _strided(v, gpu):
    """the same values as a view with a stride of two rows"""
    import torch

    big = torch.full((2 * v.shape[0],) + v.shape[1:], float("nan"), dtype=torch.float64, device=gpu)
    big[::2] = _contiguous(v, gpu)
    view = big[::2]
    assert not view.is_contiguous() or v.shape[0] < 2
    return view


def _flat(o):
    """the tensors of a method's result, in order"""
    import torch

    if isinstance(o, torch.Tensor):
        return [o]
    return [t for part in (o.values() if isinstance(o, dict) else o) if part is not None for t in _flat(part)]


def _one(bodies):
    return dict(bodies=[bodies - 1], offsets=[EP.OFFSET])


# method -> [(case, model, the tensor arguments (keys of the inputs), the ones written in place, call(plan, x, stream))]
ROWS = [
    ("forward_dynamics", "chain", ("q", "qd", "tau"), (), lambda p, x, s: p.forward_dynamics(x["q"], x["qd"], x["tau"], stream=s)),
    ("forward_dynamics-f_ext-out", "chain", ("q", "qd", "tau", "fext", "out"), ("out",),
     lambda p, x, s: p.forward_dynamics(x["q"], x["qd"], x["tau"], out=x["out"], stream=s, f_ext=x["fext"])),
    ("inverse_dynamics", "chain", ("q", "qd", "tau"), (), lambda p, x, s: p.inverse_dynamics(x["q"], x["qd"], x["tau"], stream=s)),
    ("inverse_dynamics-f_ext-out", "chain", ("q", "qd", "tau", "fext", "out"), ("out",),
     lambda p, x, s: p.inverse_dynamics(x["q"], x["qd"], x["tau"], out=x["out"], stream=s, f_ext=x["fext"])),
    ("bias_force", "chain", ("q", "qd", "fext"), (), lambda p, x, s: p.bias_force(x["q"], x["qd"], stream=s, f_ext=x["fext"])),
    ("mass_matrix", "chain", ("q",), (), lambda p, x, s: p.mass_matrix(x["q"], stream=s)),
    ("fd_dtau", "chain", ("q",), (), lambda p, x, s: p.fd_dtau(x["q"], stream=s)),
    ("fd_dqd", "chain", ("q", "qd", "tau"), (), lambda p, x, s: p.fd_dqd(x["q"], x["qd"], x["tau"], stream=s)),
    ("fd_dq", "chain", ("q", "qd", "tau"), (), lambda p, x, s: p.fd_dq(x["q"], x["qd"], x["tau"], stream=s)),
    ("fd_derivatives", "chain", ("q", "qd", "tau"), (), lambda p, x, s: p.fd_derivatives(x["q"], x["qd"], x["tau"], stream=s)),
    ("id_derivatives", "chain", ("q", "qd", "tau"), (), lambda p, x, s: p.id_derivatives(x["q"], x["qd"], x["tau"], stream=s)),
    ("spanning", "chain", ("q", "qd", "tau"), (), lambda p, x, s: p.spanning(x["q"], x["qd"], x["tau"], stream=s)),
    ("integrate", "chain", ("q", "qd", "tau"), (), lambda p, x, s: p.integrate(x["q"], x["qd"], x["tau"], DT, stream=s)),
    ("integrate-out", "chain", ("q", "qd", "tau", "q_next", "out"), ("q_next", "out"),
     lambda p, x, s: p.integrate(x["q"], x["qd"], x["tau"], DT, out=(x["q_next"], x["out"]), stream=s)),
    ("step", "chain", ("q", "qd", "tau", "fext"), (), lambda p, x, s: p.step(x["q"], x["qd"], x["tau"], DT, f_ext=x["fext"], stream=s)),
    ("rollout", "chain", ("q", "qd", "tau"), (), lambda p, x, s: p.rollout(x["q"], x["qd"], x["tau"], DT, T, stream=s)),
    ("rollout-per-step-record", "chain", ("q", "qd", "tau_T"), (),
     lambda p, x, s: p.rollout(x["q"], x["qd"], x["tau_T"], DT, T, record=True, stream=s)),
    ("body_poses", "chain", ("q",), (), lambda p, x, s: p.body_poses(x["q"], stream=s)),
    ("body_twists", "chain", ("q", "qd", "tau"), (), lambda p, x, s: p.body_twists(x["q"], x["qd"], x["tau"], stream=s)),
    ("apply_test_force", "chain", ("q", "force"), (),
     lambda p, x, s: p.apply_test_force(x["q"], p.n_bodies - 1, EP.OFFSET, x["force"], stream=s)),
    ("inv_osim", "chain", ("q",), (), lambda p, x, s: p.inv_osim(x["q"], with_jacobian=True, stream=s, **_one(p.n_bodies))),
    ("energy", "chain", ("q", "qd"), (), lambda p, x, s: p.energy(x["q"], x["qd"], stream=s)),
    ("centroidal", "chain", ("q", "qd", "tau"), (), lambda p, x, s: p.centroidal(x["q"], x["qd"], x["tau"], stream=s)),
    ("centroidal_matrix", "chain", ("q",), (), lambda p, x, s: p.centroidal_matrix(x["q"], stream=s)),
    ("time_kernel", "chain", ("q", "qd", "tau", "out"), ("out",),
     lambda p, x, s: [x["out"]] if p.time_kernel("aba", x["q"], x["qd"], x["tau"], x["out"], iters=1, stream=s) >= 0 else None),
    ("sharded_device", "chain", ("q", "qd", "tau"), (),
     lambda p, x, s: p.sharded_device("aba", [x["q"]], [x["qd"]], [x["tau"]], streams=None if s is None else [s])[0]),
    ("sharded_device-gathered", "chain", ("q", "qd", "tau", "out"), ("out",),
     lambda p, x, s: p.sharded_device("rnea", [x["q"]], [x["qd"]], [x["tau"]], gathered=x["out"], streams=None if s is None else [s])[1]),
    ("project_positions", "tello_with_arms", ("q_start",), ("q_start",),
     lambda p, x, s: (x["q_start"], p.project_positions(x["q_start"], stream=s))),
    ("state_to_independent", "tello_with_arms", ("q", "qd"), (),
     lambda p, x, s: p.state_to_independent(x["q"], x["qd"], want_gmax=True, stream=s)),
    ("constraint_gain", "tello_with_arms", ("q",), (), lambda p, x, s: p.constraint_gain(x["q"], stream=s)),
    ("contact_points", "tello_with_arms", ("q", "qd", "tau"), (),
     lambda p, x, s: p.contact_points(x["q"], qd=x["qd"], ydd=x["tau"], stream=s, **_one(p.n_bodies))),
    ("contact_dynamics", "tello_with_arms", ("q", "qd", "tau", "a_des", "fext"), (),
     lambda p, x, s: p.contact_dynamics(x["q"], x["qd"], x["tau"], a_des=x["a_des"], f_ext=x["fext"], stream=s, **_one(p.n_bodies))),
    ("contact_impulse", "tello_with_arms", ("q", "qd", "a_des"), (),
     lambda p, x, s: p.contact_impulse(x["q"], x["qd"], v_des=x["a_des"], restitution=0.25, stream=s, **_one(p.n_bodies))),
]
IDS = [r[0] for r in ROWS]


def test_every_method_has_a_row():
    takes_tensors = {name for name, f in vars(G.Plan).items() if callable(f) and not name.startswith("_")
                     and {"stream", "streams"} & set(inspect.signature(f).parameters)}
    assert takes_tensors and takes_tensors <= {case.split("-")[0] for case in IDS}, takes_tensors - {case.split("-")[0] for case in IDS}


def _args(model, keys, gpu, make=_contiguous, **other):
    """fresh tensors for one call (an in-place call may write to them): keys made by `make`, those in `other` by their own maker"""
    host = _host_inputs(model)
    return {k: other.get(k, make)(host[k], gpu) for k in keys}


_REFERENCE = {}


def _reference(case, gpu):
    """the outputs of the row's call on contiguous tensors on the current stream: made once per row"""
    import torch

    if case not in _REFERENCE:
        _, model, keys, _, call = ROWS[IDS.index(case)]
        _REFERENCE[case] = [o.clone() for o in _flat(call(G.Plan(_blob(model)), _args(model, keys, gpu), None))]
        torch.cuda.synchronize()
        assert _REFERENCE[case] and all(bool(torch.isfinite(o).all()) for o in _REFERENCE[case] if o.is_floating_point())
    return _REFERENCE[case]


def _same(got, want):
    import torch

    torch.cuda.synchronize()
    got = _flat(got)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and torch.equal(g, w), f"output {i} differs from the call on contiguous tensors"


@pytest.mark.parametrize("case,model,keys,fixed,call", ROWS, ids=IDS)
def test_strided_inputs_give_the_same_bits(case, model, keys, fixed, call, gpu):
    plan = G.Plan(_blob(model))
    x = _args(model, keys, gpu, _strided, **{k: _contiguous for k in fixed})
    _same(call(plan, x, None), _reference(case, gpu))
    for k in fixed:  # a tensor the call writes to is taken as it is or not at all
        with pytest.raises((ValueError, G.GrbdaError)):
            call(plan, _args(model, keys, gpu, **{k: _strided}), None)


def _bad(model, keys, gpu):
    """(what is wrong, the exception it raises, the arguments) for every tensor argument and every class of fault"""
    import torch

    for k in keys:
        yield f"{k} on the host", G.GrbdaError, _args(model, keys, gpu, **{k: lambda v, d: _contiguous(v, d).cpu()})
        yield f"{k} int64", G.GrbdaError, _args(model, keys, gpu, **{k: lambda v, d: _contiguous(v, d).long()})
        if len(keys) > 1:
            yield f"{k} float32 among float64", TypeError, _args(model, keys, gpu, **{k: lambda v, d: _contiguous(v, d).to(torch.float32)})
        yield f"{k} short by a column", ValueError, _args(model, keys, gpu, **{k: lambda v, d: _contiguous(v, d)[..., :-1]})


@pytest.mark.parametrize("case,model,keys,fixed,call", ROWS, ids=IDS)
def test_bad_arguments_raise_by_one_rule_and_enqueue_nothing(case, model, keys, fixed, call, gpu):
    plan = G.Plan(_blob(model))  # a fresh plan: its first device work is the good call below
    for what, exc, x in _bad(model, keys, gpu):
        with pytest.raises(exc) as e:
            call(plan, x, None)
        assert type(e.value) is exc, f"{what}: {type(e.value).__name__}"
        if exc is G.GrbdaError:
            assert e.value.code == -3 and "no CPU fallback" in str(e.value), what
    first = [o.clone() for o in _flat(call(plan, _args(model, keys, gpu), None))]
    _same(call(plan, _args(model, keys, gpu), None), first)
    _same(first, _reference(case, gpu))


@pytest.mark.parametrize("case,model,keys,fixed,call", ROWS, ids=IDS)
def test_a_side_stream_gives_the_same_bits(case, model, keys, fixed, call, gpu):
    import torch

    want = _reference(case, gpu)
    plan = G.Plan(_blob(model))
    x = _args(model, keys, gpu, _strided, **{k: _contiguous for k in fixed})
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))  # (the inputs were written on the current stream)
    got = call(plan, x, side)
    side.synchronize()
    _same(got, want)
