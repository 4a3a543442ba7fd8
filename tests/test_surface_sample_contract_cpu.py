"""CPU: the contract of the surface sampler (csrc/surface_sample_core.h) on the host emulation built from that header
(tests/surface_sample_emul.cpp): the same bits for every forced block and for a shuffled job order; a launch of several objects
equals the single launches; a failed object is NaN / -1 and leaves its neighbours alone; a face without area is never drawn; every
sample lies on its face (float64); the drawn faces and points against a float64 restatement of trimesh's algorithm on the same
uniforms; the face counts against their binomial expectation; and the arguments the launch refuses.  The GPU test holds the kernels
against this emulation bit for bit."""
import numpy as np
import pytest

from support import surface_sample as ss


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])


GOOD = [n for n in ss.meshes() if n not in ss.FAILED]


def test_limits_are_what_the_documents_say():
    assert ss.limits() == dict(block_step=64, max_block=2048, default_block=2048, max_blocks=2048, max_faces=1 << 22)


@pytest.mark.parametrize("name", sorted(ss.meshes()))
def test_same_bits_for_every_block_and_job_order(name):
    mesh = ss.meshes()[name]
    for count in ss.COUNTS:
        want = ss.emul_case(name, count, 0)
        for block in ss.BLOCKS[1:]:
            assert _same(ss.emul_case(name, count, block), want), (name, count, block)
    n_jobs = int(ss.prefix([0, len(mesh[0])], [0, len(mesh[1])], 65, 64)[-1])
    order = np.random.RandomState(3).permutation(n_jobs)
    assert _same(ss.emul_one(mesh, ss.case_uniforms(name, 65), 64, job_order=order), ss.emul_case(name, 65, 0))
    assert _same(ss.emul_one(mesh, ss.case_uniforms(name, 65), 64, job_order=np.arange(n_jobs)[::-1]), ss.emul_case(name, 65, 0))


@pytest.mark.parametrize("block", ss.BLOCKS)
def test_several_objects_equal_the_single_launches(block):
    for count in (1, 65, 4096):
        packed, u, (points, face) = ss.multi_case(count, block)
        n_jobs = int(ss.prefix(packed[2], packed[3], count, block)[-1])
        shuffled = ss.emul(*packed, u, block, job_order=np.random.RandomState(count).permutation(n_jobs))
        assert _same(shuffled, (points, face))
        for o, name in enumerate(ss.MULTI):
            assert _same((points[o], face[o]), ss.emul_case(name, count, block)), (name, count, block)
            if name in ss.FAILED:
                assert np.isnan(points[o]).all() and (face[o] == -1).all()
            else:
                assert np.isfinite(points[o]).all() and (face[o] >= 0).all() and (face[o] < len(ss.meshes()[name][1])).all()


def test_failed_objects():
    for name in ss.FAILED:
        points, face = ss.emul_case(name, 65, 0)
        assert np.isnan(points).all() and (face == -1).all()
    # no area at all: one triangle of three equal vertices, and one of three collinear ones
    v = np.asarray([[0.5, 0.25, 0.0]] * 3 + [[0.0, 0.0, 0.0], [0.25, 0.5, 0.0], [0.5, 1.0, 0.0]], np.float32)
    points, face = ss.emul_one((v, np.asarray([[0, 1, 2], [3, 4, 5]], np.int32)), ss.uniforms((7,), 1))
    assert np.isnan(points).all() and (face == -1).all()
    # a NaN vertex no face refers to does not fail the object; an infinite one that a face refers to does
    v, f = ss.meshes()["soup_2"]
    spare = np.concatenate([v, [[np.nan, 0.0, 0.0]]]).astype(np.float32)
    assert _same(ss.emul_one((spare, f), ss.case_uniforms("soup_2", 65)), ss.emul_case("soup_2", 65, 0))
    inf = v.copy()
    inf[4, 2] = np.inf
    assert np.isnan(ss.emul_one((inf, f), ss.uniforms((3,), 1))[0]).all()
    # edges that overflow fp32 give a weight that is not finite
    big = (v * np.float32(3e38)).astype(np.float32)
    assert np.isfinite(big).all() and (ss.emul_one((big, f), ss.uniforms((3,), 1))[1] == -1).all()


def test_a_face_without_weight_is_never_drawn():
    for name in ("degenerate", "spanning"):
        mesh = ss.meshes()[name]
        _, face, w, q = ss.emul_one(mesh, ss.uniforms((4096,), 5, edges=True), 64, with_weights=True)
        assert (q[face] > 0).all()
    v, f = ss.meshes()["degenerate"]
    _, _, w, q = ss.emul_one((v, f), ss.uniforms((1,), 5), with_weights=True)
    assert (w[2::3] == 0).all() and (q[2::3] == 0).all() and (w.reshape(-1, 3)[:, :2] > 0).all() and q.max() < 1 << 40 and q.max() >= 1 << 39
    # more than 2^40 times smaller than the largest: weight 0, never drawn, though its fp32 area is positive
    tri = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    v = np.concatenate([tri * 2.0 ** -21, tri, tri * 2.0 ** -19]).astype(np.float32)
    u = ss.uniforms((4096,), 6, edges=True)
    _, face, w, q = ss.emul_one((v, np.arange(9, dtype=np.int32).reshape(3, 3)), u, with_weights=True)
    assert w[0] == 2.0 ** -42 and q[0] == 0 and q[1] == 1 << 39 and q[2] == 2 and not (face == 0).any() and face[0] == 1


@pytest.mark.parametrize("name", GOOD)
def test_every_sample_lies_on_its_face(name):
    v, f = ss.meshes()[name]
    for count in ss.COUNTS:
        points, face = ss.emul_case(name, count, 0)
        lowest, largest_sum, dist, _ = ss.on_face(v, f, points, face)
        print(f"{name} count {count}: lowest barycentric {lowest:.3e}, largest r1 + r2 - 1 {largest_sum - 1:.3e}, plane distance / extent "
              f"{dist / ss.extent(v):.3e}")
        assert lowest >= -ss.ON_FACE and largest_sum <= 1.0 + ss.ON_FACE and dist <= ss.ON_FACE * ss.extent(v), (name, count)


@pytest.mark.parametrize("name", GOOD)
def test_against_the_float64_restatement_of_trimesh(name):
    v, f = ss.meshes()[name]
    assert len(f) <= 4097
    u = ss.uniforms((4096,), seed=len(f) + 17)
    points, face = ss.emul_one((v, f), u, 0)
    want_points, want_face = ss.trimesh_sample(v, f, u)
    differ = face != want_face
    agree = ~differ
    err = np.abs(points[agree].astype(np.float64) - want_points[agree]).max()
    print(f"{name}: {int(differ.sum())} of {len(u)} faces differ (F * 2^-22 = {len(f) * 2.0 ** -22:.2e}); points differ by {err / ss.extent(v):.3e} of the extent")
    assert differ.mean() <= ss.FACE_CAP
    assert err <= ss.ON_FACE * ss.extent(v)


def _binomial_ok(counts, p, n):
    return np.abs(counts - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p))


def test_face_counts_follow_the_areas():
    v, f = ss.meshes()["cube"]
    n = 4096 * 12
    _, face = ss.emul_one((v, f), ss.uniforms((n,), 21))
    counts = np.bincount(face, minlength=12)
    print("cube:", counts.tolist())
    assert _binomial_ok(counts, 1.0 / 12.0, n).all()
    v, f = ss.meshes()["spanning"]
    _, face = ss.emul_one((v, f), ss.uniforms((n,), 22))
    vd = v.astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(vd[f[:, 1]] - vd[f[:, 0]], vd[f[:, 2]] - vd[f[:, 0]]), axis=1)
    p = area / area.sum()
    big = np.argsort(-p)
    big = big[: int(np.searchsorted(np.cumsum(p[big]), 0.99)) + 1]        # the faces that hold 99 % of the area
    counts = np.bincount(face, minlength=len(f))
    print(f"spanning: {len(big)} faces hold 99 % of the area; their counts {counts[big].tolist()}")
    assert len(big) >= 10 and _binomial_ok(counts[big], p[big], n).all()


def test_scratch_refuses_bad_arguments():
    ok = ss.prefix([0, 8, 16], [0, 12, 24], 1, 0)
    assert ok is not None and ok.tolist() == [0, 1, 2]
    assert ss.prefix([0, 8], [0, 300], 1, 64).tolist() == [0, 5] and ss.prefix([0, 8], [0, 1 << 22], 1, 0).tolist() == [0, 2048]
    for vert_off, face_off, count, block in (
            ([0, 8, 16], [0, 12, 24], 0, 0),            # count < 1
            ([0, 8, 16], [0, 12, 12], 1, 0),            # an empty object
            ([0, 8, 16], [0, 12, 6], 1, 0),             # face offsets descend
            ([0, 8, 4], [0, 12, 24], 1, 0),             # vertex offsets descend
            ([1, 8, 16], [0, 12, 24], 1, 0),            # do not start at 0
            ([0, 8, 16], [2, 12, 24], 1, 0),
            ([0, 8], [0, (1 << 22) + 1], 1, 0),         # more than 2^22 faces
            ([0, 8], [0, 64 * 2048 + 1], 1, 64),        # more than 2048 blocks of a forced size
            ([0, 8, 16], [0, 12, 24], 1, 32), ([0, 8, 16], [0, 12, 24], 1, 96), ([0, 8, 16], [0, 12, 24], 1, 4096),
            ([0, 8, 16], [0, 12, 24], 1, -64)):
        assert ss.prefix(vert_off, face_off, count, block) is None, (vert_off, face_off, count, block)
