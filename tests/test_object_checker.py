"""tptObjectPlaneDevice and tptTemporalAccumulateObjectsDevice without a GPU: their CPU statements -- tests/object_checker.c and
object_lib's numpy twins -- agree byte for byte on seeded cases, and the statement has the properties include/tpt_hip.h promises: with
no table and one constant id it is tptTemporalAccumulateDevice, a tap of another object is never counted, an entry's .w caps the
history, an id outside the table reads no entry, and an object that moved is found where it stood."""
import numpy as np
import pytest

from object_lib import KINDS, ObjectChecker, moved_sphere_case, object_numpy, object_plane_numpy, synthetic_objects
from oracle_lib import FLAG_ANIMATE, Oracle
from temporal_lib import TemporalChecker, synthetic_case

f32 = np.float32
NAMES = ("colour", "albedo", "moments", "variance")
SIZES = [(1, 1), (17, 1), (1, 17), (8192, 2), (130, 67)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return ObjectChecker(tmp_path_factory.mktemp("object_checker"))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return TemporalChecker(tmp_path_factory.mktemp("temporal_checker"))


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_checker_and_numpy_agree(checker, kind, size):
    w, h = size
    cam, cur, obj, prev, motion = synthetic_objects(kind, w, h)
    for kw in (dict(max_history=8.0), dict(max_history=2.5, depth_tolerance=0.5, normal_tolerance=1.0, coverage_tolerance=0.25)):
        for table in (motion, None):
            got, want = checker.run(cam, cur, obj, prev, table, **kw), object_numpy(cam, cur, obj, prev, table, **kw)
            for name, g, n in zip(NAMES, got, want):
                assert g.tobytes() == n.tobytes(), (name, kw, table is None)
            N = got[2][..., 3]
            assert (N >= 1).all() and (N <= kw["max_history"]).all()
            if kind in ("first", "behind"):
                assert (N == 1).all()
    if kind == "same" and size == (130, 67):
        assert (checker.run(cam, cur, obj, prev, None)[2][..., 3] > 1).mean() > 0.3  # (the planted history is found)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_no_table_and_one_id_is_the_plain_pass(checker, plain, kind, size):
    w, h = size
    cam, cur, prev = synthetic_case(kind, w, h)
    for const in (-1, 0, 7):
        ids = np.full((h, w), const, np.int32)
        got = checker.run(cam, cur, ids, None if prev is None else tuple(prev) + (ids,), None, max_history=8.0)
        assert same(got, plain.run(cam, cur, prev, max_history=8.0)), const


def test_a_tap_of_another_object_is_never_counted(checker, plain):
    w, h = 40, 24
    cam, cur, prev = synthetic_case("moved", w, h)  # (fractional taps)
    obj = np.full((h, w), 3, np.int32)
    other = np.full((h, w), 4, np.int32)
    got = checker.run(cam, cur, obj, tuple(prev) + (other,), None)
    assert (got[2][..., 3] == 1).all() and got[0].tobytes() == cur[0].tobytes()
    # a previous plane that differs in one column: exactly the pixels with a counted tap there change
    base = plain.run(cam, cur, prev)
    assert (base[2][..., 3] > 1).any()
    pobj = obj.copy()
    pobj[:, 20] = -1
    got = checker.run(cam, cur, obj, tuple(prev) + (pobj,), None)
    changed = np.array([g.view(np.uint32) != b.view(np.uint32) for g, b in zip(got, base)]).any(axis=(0, 3))
    assert changed.any() and not changed[:, :18].any() and not changed[:, 23:].any()
    # every rule is about equality alone: misses (-1) take history from misses
    miss = np.full((h, w), -1, np.int32)
    assert same(checker.run(cam, cur, miss, tuple(prev) + (miss,), None), base)


@pytest.mark.parametrize("cap,bound", [(1.0, 1.0), (2.0, 2.0), (0.0, 4.0), (0.5, 4.0), (2.5, 2.5), (9.0, 4.0)])
def test_an_entry_caps_the_history(checker, cap, bound):
    w, h = 40, 24
    cam, cur, prev = synthetic_case("same", w, h)
    cur[1][..., 3] = 1  # every pixel a hit: an entry is read only where c > 0
    prev[2][..., 3] = 1
    prev[4][..., 3] = 6  # a long history everywhere
    ids = np.zeros((h, w), np.int32)
    table = np.array([[0, 0, 0, cap]], f32)
    N = checker.run(cam, cur, ids, tuple(prev) + (ids,), table, max_history=4.0)[2][..., 3]
    found = checker.run(cam, cur, ids, tuple(prev) + (ids,), None, max_history=4.0)[2][..., 3] > 1
    assert found.mean() > 0.75  # (synthetic_case plants eight kinds of bad history in n / 40 pixels each: at most a fifth)
    assert (N[found] == f32(bound)).all() and (N[~found] == 1).all()
    if bound == 1.0:  # a cap of 1: this frame alone
        assert checker.run(cam, cur, ids, tuple(prev) + (ids,), table)[0].tobytes() == cur[0].tobytes()


def test_sky_pixels_read_no_entry(checker):
    w, h = 40, 24
    cam, cur, prev = synthetic_case("same", w, h)
    ids = np.zeros((h, w), np.int32)
    table = np.array([[0.3, 0.1, -0.2, 1.0]], f32)
    got = checker.run(cam, cur, ids, tuple(prev) + (ids,), table)
    want = checker.run(cam, cur, ids, tuple(prev) + (ids,), None)
    sky = cur[1][..., 3] == 0
    assert sky.any() and (~sky).any()
    for g, n in zip(got, want):
        assert g[sky].tobytes() == n[sky].tobytes()
    assert (got[2][..., 3][~sky] == 1).all()  # (the hits are capped at 1, or moved off their history)


def test_an_id_outside_the_table_reads_no_entry(checker):
    w, h = 40, 24
    cam, cur, prev = synthetic_case("moved", w, h)
    table = np.array([[0.3, 0.1, -0.2, 1.0], [0.5, 0.5, 0.5, 1.0]], f32)
    want = None
    for const in (-1, 2, 3, 65534, 2 ** 31 - 1, -2 ** 31):
        ids = np.full((h, w), const, np.int32)
        got = checker.run(cam, cur, ids, tuple(prev) + (ids,), table)
        none = checker.run(cam, cur, ids, tuple(prev) + (ids,), None)
        assert same(got, none), const
        want = want or none
        assert same(got, want)
    ids = np.ones((h, w), np.int32)  # (and an id inside it does)
    assert not same(checker.run(cam, cur, ids, tuple(prev) + (ids,), table), want)


def test_a_moved_object_is_found_where_it_stood(checker, plain):
    w, h = 96, 54
    cam, cur, obj, prev, motion = moved_sphere_case(w, h)
    on = obj == 0
    assert on.sum() > 100 and (prev[5] == 0).sum() > 100 and (on & (prev[5] != 0)).sum() > 30
    followed = checker.run(cam, cur, obj, prev, motion)[2][..., 3]
    plain_n = plain.run(cam, cur, prev[:5])[2][..., 3]
    unfollowed = checker.run(cam, cur, obj, prev, None)[2][..., 3]
    n_new, n_plain, n_ids = int((followed[on] == 2).sum()), int((plain_n[on] == 2).sum()), int((unfollowed[on] == 2).sum())
    print("N == 2 on the sphere: followed %d, plain pass %d, ids without the table %d, of %d" % (n_new, n_plain, n_ids, int(on.sum())))
    assert n_new > n_plain and n_new > n_ids
    # where the plain reprojection lands off the previous footprint there is history only with the table
    off = on & (prev[5] != 0)
    assert (plain_n[off] == 1).all() and (followed[off] == 2).any()
    # the interior of the sphere is found whole: what is missed lies on the rim
    assert n_new > 0.8 * on.sum()


def test_object_plane_checker_and_numpy_agree(checker):
    o = Oracle.get()
    spheres, _ = o.default_scene()
    for w, h in SIZES:
        cams = np.concatenate([o.default_camera(w, h), o.camera((2.5, 1.5, 2.0), (0, 0, 0), (0, 1, 0), 50.0, w / h, 0.1, 3.0)])
        got = checker.plane(spheres, cams, w, h)
        for j in range(2):
            assert got[j].tobytes() == object_plane_numpy(spheres, cams[j:j + 1], w, h).tobytes(), (w, h, j)
    assert set(np.unique(got)) > {-1, 0}  # (sky, ground and spheres at the last size)


def test_object_plane_animates_like_update(checker):
    o = Oracle.get()
    spheres, _ = o.default_scene()
    w, h = 130, 67
    cam = o.default_camera(w, h)
    times = np.array([0.0, 1.25, np.nan], f32)
    cams = np.concatenate([cam] * 3)
    got = checker.plane(spheres, cams, w, h, times, FLAG_ANIMATE)
    for j in range(2):
        moved = spheres.copy()
        o.animate(moved, float(times[j]))
        assert got[j].tobytes() == object_plane_numpy(moved, cam, w, h).tobytes()
    assert got[0].tobytes() != got[1].tobytes()
    assert not np.isin(got[2], (1, 8)).any() and np.isin(got[1], (1, 8)).any()  # (a NaN time: the two spheres are nowhere)
    # without the flag, without times, or with 8 spheres nothing moves
    still = checker.plane(spheres, cam, w, h)
    assert checker.plane(spheres, cams, w, h, times, 0)[1].tobytes() == still[0].tobytes()
    eight = checker.plane(spheres[:8], cams, w, h, times, FLAG_ANIMATE)
    assert eight[1].tobytes() == checker.plane(spheres[:8], cam, w, h)[0].tobytes()
    nine = checker.plane(spheres[:9], cams, w, h, times, FLAG_ANIMATE)
    assert nine[1].tobytes() != checker.plane(spheres[:9], cam, w, h)[0].tobytes()


def test_object_plane_ties_and_the_far_root(checker):
    o = Oracle.get()
    spheres, _ = o.default_scene()
    w, h = 64, 36
    cam = o.default_camera(w, h)
    twice = np.concatenate([spheres[:9], spheres[5:6], spheres[9:]])  # sphere 5 again at index 9
    got = checker.plane(twice, cam, w, h)[0]
    assert (got == 5).any() and not (got == 9).any()
    assert got.tobytes() == object_plane_numpy(twice, cam, w, h).tobytes()
    inside = o.camera((0.5, 1.0, 0.5), (0, 0, 0), (0, 1, 0), 60.0, w / h, 0.0, 3.0)  # the centre of the glass sphere (7)
    got = checker.plane(spheres, inside, w, h)[0]
    assert (got == 7).all()
    assert got.tobytes() == object_plane_numpy(spheres, inside, w, h).tobytes()
