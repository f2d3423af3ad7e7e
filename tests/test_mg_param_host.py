"""CPU checks of the parametrised Moore-Greitzer plant's restatement (tests/mg_param_ref.py) and of
the Python helpers around bqp_closed_loop.plant_par: at the nominal coefficients the restatement is
oracle.mg_model's plant bit for bit, bqp.mg_plant_params maps the physical parameters as
documented, a step from bqp.mg_steady_state stays there, and a +-10 % parameter draw moves a step
by far more than the bars the GPU comparisons use (tests/test_gpu_plant_par.py)."""
import numpy as np
import pytest

import mg_param_ref as M
from oracle.mg_model import TS, U_WP, X_WP, mg_ode23, mg_rk4

NS = 2000


@pytest.fixture(scope='module')
def samples():
    rng = np.random.default_rng(20250)
    x = X_WP + rng.uniform(-1, 1, (NS, 4)) * np.array([0.3, 0.3, 0.3, 2.0])
    u = U_WP + rng.uniform(-1, 1, NS)
    return x, u


def test_rk4_equals_oracle_at_nominal(samples):
    x, u = samples
    bad = sum(not np.array_equal(M.mg_rk4_p(M.NOMINAL, TS, x[i], u[i]), mg_rk4(TS, x[i], u[i]))
              for i in range(NS))
    assert bad == 0, bad


def test_ode23_equals_oracle_at_nominal(samples):
    x, u = samples
    bad = 0
    for i in range(NS):
        y, errs = M.mg_ode23_p(M.NOMINAL, TS, x[i], u[i])
        assert len(errs) >= 10                       # MaxStep is delta / 10
        bad += not np.array_equal(y, mg_ode23(TS, x[i], u[i]))
    assert bad == 0, bad


def test_mg_plant_params():
    import bqp
    p = bqp.mg_plant_params()
    assert p.shape == (4,) and p.dtype == np.float64 and p.flags.c_contiguous
    assert np.array_equal(p, M.NOMINAL)
    assert np.array_equal(p, [0.0, 1.0, 1000.0, 2.0 * np.sqrt(500.0)])
    # wn, zeta fill wn^2 and 2 zeta wn; beta enters as 1 / beta^2
    q = bqp.mg_plant_params(x2_c=0.03, beta=1.25, wn=30.0, zeta=0.6)
    assert np.array_equal(q, [0.03, 1.0 / (1.25 * 1.25), 900.0, 2.0 * 0.6 * 30.0])
    q = bqp.mg_plant_params(wn2=900.0, zeta=0.5)
    assert np.array_equal(q, [0.0, 1.0, 900.0, 2.0 * 0.5 * np.sqrt(900.0)])
    q = bqp.mg_plant_params(wn=31.0)
    assert np.array_equal(q, [0.0, 1.0, 961.0, 2.0 * np.sqrt(500.0)])
    # broadcasting: (3, 1) against (2,) -> (3, 2, 4)
    q = bqp.mg_plant_params(x2_c=np.array([[0.0], [0.01], [0.02]]), wn2=np.array([900.0, 1100.0]))
    assert q.shape == (3, 2, 4) and q.flags.c_contiguous
    assert np.array_equal(q[1, 0], [0.01, 1.0, 900.0, 2.0 * np.sqrt(500.0)])
    assert np.array_equal(q[2, 1], [0.02, 1.0, 1100.0, 2.0 * np.sqrt(500.0)])


def test_plant_params_shapes():
    from bqp.loop import _plant_params
    b, steps = 3, 5
    for shape, want in (((4,), (0, 0)), ((b, 4), (4, 0)), ((steps, 4), (0, 1)),
                        ((b, steps, 4), (steps * 4, 1))):
        a, stride, sched = _plant_params(np.zeros(shape), b, steps)
        assert (stride, sched) == want and a.flags.c_contiguous, shape
    # batch == steps: (steps, 4) is the schedule shared by the batch, as nmpc._schedule reads its own
    assert _plant_params(np.zeros((5, 4)), 5, 5)[1:] == (0, 1)
    for shape in ((3,), (2, 4), (b, steps, 3), (steps, b, 4)):
        with pytest.raises(ValueError):
            _plant_params(np.zeros(shape), b, steps)
    # the ClosedLoop structure's trailing members default to the nominal plant
    from bqp.loop import ClosedLoop
    cl = ClosedLoop(1, 2, 0.01, None, None)
    assert not cl.plant_par and cl.splant_par == 0 and cl.plant_par_sched == 0


def test_steady_state_and_parameter_effect(samples):
    """A step from the drawn plant's own steady state stays there (<= 1e-14).  The parameter effect:
    a step of the drawn plant differs from the nominal plant's by at least 1e-5, taken from the
    2,000 seeded states and inputs of the nominal comparison above, the kind of state the loops
    visit.  From the drawn plant's steady state only x2_c separates the two plants (there
    x[0] + 1 = x[2] sqrt(x[1]), x[3] = 0 and u = x[2], so 1/beta^2, wn^2 and 2 zeta wn multiply zeros): the difference
    is delta |x2_c|, which 2,000 uniform draws of x2_c bring to 1e-7 and below whatever the seed, so
    that figure is printed and not bounded."""
    import bqp
    x, u = samples
    rng = np.random.default_rng(20251)
    P = M.draw_params(rng, (NS,))
    x1 = rng.uniform(0.3, 0.7, NS)
    XS, US = bqp.mg_steady_state(P, x1)
    assert XS.shape == (NS, 4) and US.shape == (NS,)
    moved, effect, effect_ss = 0.0, np.inf, np.inf
    for i in range(NS):
        xs, us = M.mg_steady_state(P[i], x1[i])
        assert np.array_equal(xs, XS[i]) and us == US[i]
        xn = M.mg_rk4_p(P[i], TS, xs, us)
        moved = max(moved, np.abs(xn - xs).max())
        effect_ss = min(effect_ss, np.abs(xn - mg_rk4(TS, xs, us)).max())
        effect = min(effect, np.abs(M.mg_rk4_p(P[i], TS, x[i], u[i]) - mg_rk4(TS, x[i], u[i])).max())
    print('step from the steady state moves %.2e; smallest parameter effect %.2e (from the steady '
          'state: %.2e)' % (moved, effect, effect_ss))
    assert moved <= 1e-14, moved
    assert effect >= 1e-5, effect
    # independent of beta, wn, zeta; one params row against several x1 broadcasts
    xs, us = bqp.mg_steady_state(bqp.mg_plant_params(x2_c=0.02, beta=1.3, wn=25.0, zeta=0.4), [0.4, 0.5])
    x0, u0 = bqp.mg_steady_state(bqp.mg_plant_params(x2_c=0.02), [0.4, 0.5])
    assert xs.shape == (2, 4) and np.array_equal(xs, x0) and np.array_equal(us, u0)
