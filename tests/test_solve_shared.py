"""The solve stated once for host and device (csrc/ssd_solve.h), host side: this build's
ssd_surface_gates_from_moments, ssd_surface_fit_solve and ssd_ground_fit_solve reproduce, bit for bit, what the text they were moved
from returned (tests/golden/solve_goldens.json, written from the commit before the move), and the refusals of the new entry points that
need no device.  No GPU needed; the device side is tests/test_gpu_surface_gates.py."""
import ctypes as C

import solve_goldens as sg


def _hex(values):
    return [float(v).hex() for v in values]


def test_the_goldens_hold_what_they_say():
    d = sg.doc()
    assert len(d["written_from_commit"]) == 40 and len(d["records"]) >= 10
    assert sg.rules() == [(200, 2.5, 0.0), (1, 16.0, 0.0), (200, 2.0, 2.0 ** -10)]
    ns = [r["n_surfaces"] for r in d["records"]]
    assert 0 in ns and 17 in ns and all(len(r["s"]) == n for r, n in zip(d["records"], ns))
    # every status under every min_points, open and closed gates, a gate at gate_min and one above it, an exactly flat surface
    status = {(mp, s[0]) for r in d["records"] for mp, rows in sg.fits_of(r, "surface_fit") for s in rows}
    assert status == {(mp, st) for mp in (1, 200) for st in (0, 1, 2)}
    gm = 2.0 ** -10
    third = [float.fromhex(g[4]) for r in d["records"] for g in r["gates"][2]]
    assert any(v == gm for v in third) and any(v > gm for v in third) and any(v == 0.0 for v in third)
    first = [(g, s) for r in d["records"] for g, s in zip(r["gates"][0], sg.fits_of(r, "surface_fit")[1][1])]
    assert any(s[0] == 0 and float.fromhex(g[4]) == 0.0 and float.fromhex(g[3]) > 0.0 for g, s in first), "a flat surface: OK, rms 0"
    # scatter entries beyond 53 bits, on a rounding tie of the conversion and next to one
    wide = ties = near = 0
    for r in d["records"]:
        for n, s0, s1, s2, xx, xy, xz, yy, yz, zz, _ in r["s"]:
            s = (s0, s1, s2)
            for (i, j), v in zip([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)], (xx, xy, xz, yy, yz, zz)):
                c = abs(n * v - s[i] * s[j])
                cut = c.bit_length() - 53
                if cut > 0:
                    wide += 1
                    low = c & ((1 << cut) - 1)
                    ties += low == 1 << (cut - 1)
                    near += abs(low - (1 << (cut - 1))) == 1
    assert wide > 300 and ties >= 48 and near >= 96, (wide, ties, near)


def test_the_gates_are_the_goldens_bit_for_bit(ssd):
    for rec in sg.doc()["records"]:
        fm = sg.frame_moments(ssd, rec)
        for r, (mp, ks, gm) in enumerate(sg.rules()):
            got = ssd.surface_gates_from_moments(fm, mp, ks, gm)
            for k, want in enumerate(rec["gates"][r]):
                assert _hex(list(got.g[k].n) + [got.g[k].dist, got.g[k].gate]) == want, (rec["name"], r, k)
            assert bytes(got) == bytes(sg.gates_of(ssd, rec, r)), (rec["name"], r)


def test_the_surface_fit_and_the_ground_fit_are_the_goldens_bit_for_bit(ssd):
    cal = sg.calibration(ssd)
    for rec in sg.doc()["records"]:
        fm = sg.frame_moments(ssd, rec)
        for mp, rows in sg.fits_of(rec, "surface_fit"):
            f = ssd.surface_fit_solve(fm, cal, mp)
            assert (f.n_surfaces, f.ground) == (rec["n_surfaces"], rec["ground"])
            assert bytes(f)[8 + C.sizeof(ssd.SurfaceFit) * f.n_surfaces:] == bytes(C.sizeof(ssd.SurfaceFit) * (ssd.MAX_STEPS - f.n_surfaces))
            for k, w in enumerate(rows):
                s = f.s[k]
                got = [int(s.status), int(s.n), int(s.n_far)] + _hex(list(s.normal) + list(s.centroid) + [s.tilt, s.rms] + list(s.extent))
                assert got == w, (rec["name"], mp, k)
        for mp, rows in sg.fits_of(rec, "ground_fit"):
            for k, w in enumerate(rows):
                g = ssd.ground_fit_solve(fm.s[k].m, cal, mp)
                got = [int(g.status)] + _hex(list(g.normal) + [g.dist, g.rms, g.tilt, g.height_delta]) + [sg.cal_digest(g.cal)]
                assert got == w, (rec["name"], mp, k)


def test_the_new_entry_points_refuse_a_null_handle(ssd):
    L = ssd.lib()
    p = C.c_void_p(4096)            # never dereferenced: the handle is looked at first
    n = 4
    res, out = (ssd.FrameResult * n)(), (ssd.FrameSurfaces * n)()
    idx = (C.c_uint16 * n)()
    calls = [
        ("ssd_enqueue_surface_gates", lambda: L.ssd_enqueue_surface_gates(None, p, n, None, 200, 2.5, 0.0, p)),
        ("ssd_enqueue_surface_refit_device", lambda: L.ssd_enqueue_surface_refit_device(None, p, 64, n, None, 0, p, 200, 2.5, 0.0, p)),
        ("ssd_enqueue_cameras_surface_refit_device", lambda: L.ssd_enqueue_cameras_surface_refit_device(None, p, 64, n, None, 0, p, 200, 2.5, 0.0, p)),
        ("ssd_process_host_surfaces_refit_device", lambda: L.ssd_process_host_surfaces_refit_device(None, p, n, 0, res, None, None, 200, 2.5, 0.0, 1, out)),
        ("ssd_process_host_cameras_surfaces_refit_device",
         lambda: L.ssd_process_host_cameras_surfaces_refit_device(None, p, n, idx, 0, res, None, None, 200, 2.5, 0.0, 1, out)),
    ]
    for name, call in calls:
        assert name in ssd.EXPORTS and call() == -1, name
        assert name.encode() in L.ssd_last_error(), (name, L.ssd_last_error())
