"""Writes tests/golden/losses.json: rho0, rho1, rho2 of the library's loss functions (include/rsba_amd.h, rsba_loss) at 50 digits.

Imports neither the product nor the oracle.  rho0 is the branch of the table that the loss takes at s, as a function of s; rho1 and
rho2 are mpmath's numerical derivatives of THAT function, not the table's formulas for them — so the table itself is checked.

The s of every loss: 0, 1e-300, 1e-8, knee / 2, knee, 2 knee, 1e3 knee, 1e12 (knee: a^2 for HUBER, SOFT_L_ONE, CAUCHY; a for ARCTAN
and TOLERANT; 1 for TRIVIAL), and for TOLERANT the two sides of x = (s - a) / b = 36.7: x = 36.5 and x = 37, at which s and x are
exact in binary64 for the parameters below (rho2 ~ e^-x there: an x rounded in its last place would move it by 37 ulps, which is
the conditioning of the function and not an error of an implementation).

    python tests/golden/make_loss_golden.py
"""
import json
import os

import mpmath as mp

mp.mp.dps = 50

TRIVIAL, HUBER, SOFT_L_ONE, CAUCHY, ARCTAN, TOLERANT = range(6)
LOSSES = [(TRIVIAL, 0.0, 0.0, 1.0), (HUBER, 2.0, 0.0, 1.0), (SOFT_L_ONE, 10.0, 0.0, 1.0), (CAUCHY, 10.0, 0.0, 1.0), (ARCTAN, 100.0, 0.0, 1.0),
          (TOLERANT, 150.0, 50.0, 1.0), (TOLERANT, 100.0, 25.0, 1.0), (TOLERANT, 1.0, 0.5, 1.0), (TOLERANT, 4.0, 2.0, 1.0),
          (CAUCHY, 10.0, 0.0, 0.25), (TOLERANT, 100.0, 25.0, 0.5), (SOFT_L_ONE, 0.5, 0.0, 3.0), (ARCTAN, 0.25, 0.0, 1.0)]


def branch(kind, a, b, s):
    """rho0 as a function of t, the branch taken at s."""
    a, b = mp.mpf(a), mp.mpf(b)
    if kind == TRIVIAL:
        return lambda t: t
    if kind == HUBER:
        return (lambda t: 2 * a * mp.sqrt(t) - a * a) if mp.mpf(s) > a * a else (lambda t: t)
    if kind == SOFT_L_ONE:
        return lambda t: 2 * a * a * (mp.sqrt(1 + t / (a * a)) - 1)
    if kind == CAUCHY:
        return lambda t: a * a * mp.log(1 + t / (a * a))
    if kind == ARCTAN:
        return lambda t: a * mp.atan2(t, a)
    c = b * mp.log(1 + mp.exp(-a / b))
    if (mp.mpf(s) - a) / b > mp.mpf("36.7"):
        return lambda t: t - a - c
    return lambda t: b * mp.log(1 + mp.exp((t - a) / b)) - c


def values(kind, a, b):
    knee = {TRIVIAL: 1.0, HUBER: a * a, SOFT_L_ONE: a * a, CAUCHY: a * a, ARCTAN: a, TOLERANT: a}[kind]
    out = [0.0, 1e-300, 1e-8, knee / 2, knee, 2 * knee, 1e3 * knee, 1e12]
    if kind == TOLERANT:
        out += [a + 36.5 * b, a + 37.0 * b]
    return out


def main():
    cases = []
    for kind, a, b, scale in LOSSES:
        rows = []
        for s in values(kind, a, b):
            f = branch(kind, a, b, s)
            # (every branch is analytic around s, far beyond mpmath's step; its error is absolute, so the derivatives at s = 1e-300 —
            # ARCTAN's rho2 is -2e-304 there — are taken at 1 000 digits, then rounded to 50 like the rest)
            with mp.workdps(1000 if 0 < s < 1e-100 else 50):
                d = [+f(mp.mpf(s)), +mp.diff(f, mp.mpf(s), 1), +mp.diff(f, mp.mpf(s), 2)]
            rows.append(dict(s=float(s).hex(), rho=[mp.nstr(scale * v, 40) for v in d]))
        cases.append(dict(type=kind, a=a, b=b, scale=scale, rows=rows))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "losses.json")
    with open(path, "w") as fh:
        json.dump(dict(digits=50, cases=cases), fh, indent=1)
    print(path, sum(len(c["rows"]) for c in cases), "rows")


if __name__ == "__main__":
    main()
