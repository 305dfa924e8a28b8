"""Parity record of the constant-pressure dynamics over the cases of tests/test_npt_gpu.py (profiles/npt_parity.json): per
periodic fixture, mode (NPH, NPT) and batch the measured error of every compared quantity (R, V and lattice frames, E_pot,
E_kin, vol, pressure, p_eps, enthalpy of every step, the end eps) against the NumPy restatement (tests/_npt_ref.py), the
restatement's own deviation under the predictor's agreed error (noise of 1e-10 on E, F and W) and their ratio (the test
allows 1).

    python tools/npt_parity.py [--out profiles/npt_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def measure():
    import _npt_ref as nr
    from sgdml_amd.predict import GDMLPredict

    keys = nr.PARITY_KEYS + ('enthalpy',)
    cases = []
    for name in nr.PARITY_FIXTURES:
        pred = GDMLPredict(nr.parity_case(name)[0])
        for mode in ('nph', 'npt'):
            model, kw, ref, dev = nr.parity_reference(name, mode)
            dvol = nr.volume_change(kw, ref)
            for B in nr.PARITY_BATCHES:
                m = nr.parity_measure(pred, name, mode, B)
                cases.append(dict(fixture=name, mode=mode, B=B, steps=nr.PARITY_STEPS, pressure=nr.PARITY_PRESSURE,
                                  dt=kw['dt'], piston_mass=kw['piston_mass'], kT=kw['kT'],
                                  restated_volume_change=[float(dvol.min()), float(dvol.max())], measured=m))
                print(name, mode, B, ' '.join('%s %.2g' % (k, m[k]['ratio']) for k in keys), flush=True)
    worst = {k: max(c['measured'][k]['ratio'] for c in cases) for k in keys}
    return dict(bound='error <= %g x sensitivity (+ 1e-10 of the largest value for E_pot, vol, pressure and enthalpy)' %
                nr.BOUND_FACTOR,
                sensitivity='deviation of a second restated run under independent noise of 1e-10 relative on E, F and W',
                worst_error_over_allowed=worst, frames_are_the_end=all(c['measured']['frames_are_the_end'] for c in cases),
                cases=cases)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'npt_parity.json'))
    a = ap.parse_args()
    res = measure()
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(worst_error_over_allowed=res['worst_error_over_allowed'], frames_are_the_end=res['frames_are_the_end']),
                     indent=1))
