"""The forms the engine reports, step by step, and the state they leave: the step driver executes what beom_plan::plan_step
decides (beom_amd/csrc/beom_plan.h), and this holds it to what the driver did before the decision moved there.

Frame 130 x 18 (one interior tile row), the seven configurations of test_gpu_mont_history.py, each under keep_diag 0/1 and
fold_stress 0/1: steps 1..8 one call each; after every step info("uv_fused"), info("stress_folded"), info("mont_history") and
info("plain_sweeps"), after steps 4 and 8 a digest (SHA-256 over the bytes of every array of helpers.STATE as downloaded, the
sign of zero included) of the state.

TABLE and BANDS were recorded by running this module's own loops (_run, _run_bands) once on an MI355X with the library built
from the parent commit of the change that introduced beom_plan.h, named by BEOM_HIP_LIB as tools/ab.sh does; the library in the
tree has to reproduce them.  Nothing in them comes from the code under test.

The band case (130 x 99 on two bands, the frame of test_gpu_plain_sweeps.py's band test) reads the four values from each band's
engine after split steps, and checks the one refusal the change added: part 2 of a step that part 1 did not prepare."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import rough_inputs as RI
from beom_amd import capi
from helpers import STATE
from test_gpu_mont_history import CONFIGS, _fields
from test_gpu_plain_sweeps import _read, _unforced

pytestmark = pytest.mark.gpu
INFO = ("uv_fused", "stress_folded", "mont_history", "plain_sweeps")
OPTIONS = [(keep_diag, fold_stress) for keep_diag in (0, 1) for fold_stress in (0, 1)]

# (config, keep_diag, fold_stress): (the four values after each of steps 1..8, the digests after steps 4 and 8)
TABLE = {('beach_zero_visc', 0, 0): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0)),
                             ('16972e1e4a109e3c3fb0f1dc', 'ccb118cfbdc712f61651191a')),
 ('beach_zero_visc', 0, 1): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0)),
                             ('16972e1e4a109e3c3fb0f1dc', 'ccb118cfbdc712f61651191a')),
 ('beach_zero_visc', 1, 0): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0)),
                             ('16972e1e4a109e3c3fb0f1dc', 'ccb118cfbdc712f61651191a')),
 ('beach_zero_visc', 1, 1): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0)),
                             ('16972e1e4a109e3c3fb0f1dc', 'ccb118cfbdc712f61651191a')),
 ('closed_leith_3l', 0, 0): (((1, 0, 0, 3), (1, 0, 0, 3), (1, 0, 0, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3)),
                             ('1334fc77dd6b6dc23c8127b6', '6d6088764b97d74a27dd27b4')),
 ('closed_leith_3l', 0, 1): (((1, 0, 0, 3), (1, 0, 0, 3), (1, 0, 0, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3)),
                             ('1334fc77dd6b6dc23c8127b6', '6d6088764b97d74a27dd27b4')),
 ('closed_leith_3l', 1, 0): (((1, 0, 0, 1), (1, 0, 0, 1), (1, 0, 0, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1)),
                             ('53a0004a8b83f54cf4ebec96', '803596a02e79d6d2d908e298')),
 ('closed_leith_3l', 1, 1): (((1, 0, 0, 1), (1, 0, 0, 1), (1, 0, 0, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1)),
                             ('53a0004a8b83f54cf4ebec96', '803596a02e79d6d2d908e298')),
 ('island_ragged_coast', 0, 0): (((1, 0, 0, 3), (1, 0, 0, 3), (1, 0, 0, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3)),
                                 ('497c6eae4870e541f9dab5a5', '820bc9e5acd7590e36a42d5c')),
 ('island_ragged_coast', 0, 1): (((1, 0, 0, 3), (1, 0, 0, 3), (1, 0, 0, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3)),
                                 ('497c6eae4870e541f9dab5a5', '820bc9e5acd7590e36a42d5c')),
 ('island_ragged_coast', 1, 0): (((1, 0, 0, 1), (1, 0, 0, 1), (1, 0, 0, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1)),
                                 ('4ff601c047c91dfd3006457b', '74f03260ec1ae9e314614497')),
 ('island_ragged_coast', 1, 1): (((1, 0, 0, 1), (1, 0, 0, 1), (1, 0, 0, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1)),
                                 ('4ff601c047c91dfd3006457b', '74f03260ec1ae9e314614497')),
 ('jet_xyper', 0, 0): (((1, 0, 0, 3), (1, 0, 0, 3), (1, 0, 0, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3)),
                       ('fe1e845f76f7dd256b89dee6', '04138e2e1b401c7e7b4d84b3')),
 ('jet_xyper', 0, 1): (((1, 0, 0, 3), (1, 0, 0, 3), (1, 0, 0, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3)),
                       ('fe1e845f76f7dd256b89dee6', '04138e2e1b401c7e7b4d84b3')),
 ('jet_xyper', 1, 0): (((1, 0, 0, 1), (1, 0, 0, 1), (1, 0, 0, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1)),
                       ('fc68b2d889d0fe504ef15f75', 'aa9fb75089eb6c4a80521b19')),
 ('jet_xyper', 1, 1): (((1, 0, 0, 1), (1, 0, 0, 1), (1, 0, 0, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1)),
                       ('fc68b2d889d0fe504ef15f75', 'aa9fb75089eb6c4a80521b19')),
 ('sill_ocrp_nudged', 0, 0): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0)),
                              ('2718ca1720adce9f60638d3a', 'e103e1accd99753356d49697')),
 ('sill_ocrp_nudged', 0, 1): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0)),
                              ('2718ca1720adce9f60638d3a', 'e103e1accd99753356d49697')),
 ('sill_ocrp_nudged', 1, 0): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0)),
                              ('850b9e64c62bf84e8fd11795', 'f70e6877a84bcf8db01858b3')),
 ('sill_ocrp_nudged', 1, 1): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0)),
                              ('850b9e64c62bf84e8fd11795', 'f70e6877a84bcf8db01858b3')),
 ('soliton_xper', 0, 0): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3)),
                          ('048aabecf4ef431849e6809b', 'e959f58e1cd755efe8e2e84f')),
 ('soliton_xper', 0, 1): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3), (1, 0, 1, 3)),
                          ('048aabecf4ef431849e6809b', 'e959f58e1cd755efe8e2e84f')),
 ('soliton_xper', 1, 0): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1)),
                          ('048aabecf4ef431849e6809b', 'e959f58e1cd755efe8e2e84f')),
 ('soliton_xper', 1, 1): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1)),
                          ('048aabecf4ef431849e6809b', 'e959f58e1cd755efe8e2e84f')),
 ('stommel_wind_drag', 0, 0): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 2), (1, 0, 1, 2), (1, 0, 1, 2), (1, 0, 1, 2), (1, 0, 1, 2)),
                               ('ac1213db65d934355a27d5d5', '9bbf543edb3ba15ee00936e7')),
 ('stommel_wind_drag', 0, 1): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 1, 0, 2), (1, 1, 0, 2), (1, 1, 0, 2), (1, 1, 0, 2), (1, 1, 0, 2)),
                               ('6fbe6536cb7301bd3a3ca445', 'f951c638ccc427547172449c')),
 ('stommel_wind_drag', 1, 0): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0)),
                               ('ac1213db65d934355a27d5d5', '9bbf543edb3ba15ee00936e7')),
 ('stommel_wind_drag', 1, 1): (((1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0)),
                               ('ac1213db65d934355a27d5d5', '9bbf543edb3ba15ee00936e7'))}
# the four values of each of the two bands after steps 3, 4, 5, and the digests of the gathered state after steps 4 and 5
BANDS = ((((1, 0, 0, 3), (1, 0, 0, 3)), ((1, 0, 0, 3), (1, 0, 0, 3)), ((1, 0, 0, 3), (1, 0, 0, 3))), ('565485133c3ea4062c9f2faf', 'cdedfd186c0aa094dacd2083'))


def _digest(st):
    h = hashlib.sha256()
    for k in STATE:
        h.update(np.ascontiguousarray(st[k], dtype=np.float64).tobytes())
    return h.hexdigest()[:24]


def _run(config, keep_diag, fold_stress):
    f, opts, _ = _fields(config, "130x18")
    e = capi.Engine(f)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_option("keep_diag", keep_diag)
    e.set_option("fold_stress", fold_stress)
    forms, digests = [], []
    for t in range(1, 9):
        e.step(t, 1)
        forms.append(tuple(e.info(k) for k in INFO))
        if t in (4, 8):
            digests.append(_digest(e.download()))
    e.close()
    return tuple(forms), tuple(digests)


def _band_forms(many):
    return tuple(tuple(many.lib.beom_info(many.band_engine_handle(k), w.encode()) for w in INFO) for k in range(many.count))


def _bands_engine():
    g = _unforced(RI.rough_fields(_read(130, 99, 2, "leith"), 1, zero=("tt3d", "tb3d", "tu3d")))
    many = capi.MultiEngine(g, devices=[0, 0])
    assert many.count == 2
    return many


def _run_bands(many):
    forms, digests = [], []
    many.step(1, 2)
    for t in (3, 4, 5):
        many.step(t, 1)
        forms.append(_band_forms(many))
        if t >= 4:
            digests.append(_digest(many.download()))
    return tuple(forms), tuple(digests)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_forms_and_state_step_by_step(config):
    for keep_diag, fold_stress in OPTIONS:
        forms, digests = _run(config, keep_diag, fold_stress)
        want_forms, want_digests = TABLE[(config, keep_diag, fold_stress)]
        for t, (got, want) in enumerate(zip(forms, want_forms), 1):
            assert got == want, (config, keep_diag, fold_stress, "step", t, dict(zip(INFO, got)), dict(zip(INFO, want)))
        assert digests == want_digests, (config, keep_diag, fold_stress, "state after steps 4, 8")


def test_two_bands_and_a_part_of_another_step():
    many = _bands_engine()
    forms, digests = _run_bands(many)
    assert many.stats()["split"] > 0                    # the steps ran in three parts
    assert (forms, digests) == BANDS, (forms, digests)
    p, err = many.p, C.create_string_buffer(512)

    def phase(k, tstp, part):
        return many.lib.beom_step_phase(many.band_engine_handle(k), tstp, float(getattr(many.f, "tres", 0.0)), float(p.dtd8),
                                        float(p.dt_r), float(p.rsta), p.n_3d, part, err, 512)

    # step 5 is complete and no part 1 pending: a part 2 or 3 of any step is refused, and nothing ran
    for k in range(2):
        assert phase(k, 6, 2) == -3 and phase(k, 5, 3) == -3, k
        assert b"step 6" in err.value or b"step 5" in err.value, err.value
    many.sync()
    assert _band_forms(many) == forms[-1]
    assert _digest(many.download()) == digests[-1]
    # part 1 of step 6, then part 2 of step 7: refused with both steps named, and the state is where part 1 left it
    for k in range(2):
        assert phase(k, 6, 1) == 0, err.value
    many.sync()
    before = _digest(many.download())
    for k in range(2):
        assert phase(k, 7, 2) == -3, k
        assert b"step 7" in err.value and b"step 6" in err.value, err.value
    many.sync()
    assert _digest(many.download()) == before
    many.close()
