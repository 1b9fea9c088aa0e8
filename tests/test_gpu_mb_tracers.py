"""GPU checks of the mesh probes and tracers of the multi-block domains (``csrc/fg_mb_tracers.hip``, ``simulation/mb_tracers.py``,
``envs/tracers.MeshTracerMixin``) against the NumPy restatement ``tests/mb_tracers_ref.py`` and closed forms.
``B = 2``, 64 tracers and 37 probe points per env (one partly empty workgroup); ``F`` is the largest field value, ``L`` the mesh's extent."""
import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd.simulation import mb_tracers as M
from tests import helpers_mb as H
from tests import mb_tracers_ref as R

pytestmark = pytest.mark.gpu

B, N_TRACERS, N_PROBES = 2, 64, 37
EPS32 = float(np.finfo(np.float32).eps)
DTYPES = {"fp32": (torch.float32, np.float32), "fp64": (torch.float64, np.float64)}
MESHES = {"cylinder_2d": lambda: H.cylinder_2d(8), "airfoil": lambda: H.airfoil_spec(4), "twisted_ring": H.twisted_ring,
          "skewed_pair": H.skewed_pair, "split_rotated_channel": H.split_rotated_channel, "skewed_pair_3d": H.skewed_pair_3d,
          "cylinder_3d_small": H.cylinder_3d_small}
_CACHE = {}


def case(name, prec, batch=B):
    """(domain, MbPointMesh, restatement) of a mesh in a dtype, built once."""
    key = (name, prec, batch)
    if key not in _CACHE:
        dom = MESHES[name]().native(batch=batch, dtype=DTYPES[prec][0])
        _CACHE[key] = (dom, M.MbPointMesh(dom), R.RefMesh(dom, DTYPES[prec][1]))
    return _CACHE[key]


def set_fields(dom, vel, bvel, p=None):
    """Host fields ``[B, d, N]``, ``[B, d, NB]``, ``[B, N]`` into the domain; returns them as the library sees them (rounded)."""
    kw = dict(dtype=dom.dtype, device=dom.device)
    dom.velocity.copy_(torch.as_tensor(vel, **kw))
    dom.boundary_velocity[:, :, :bvel.shape[2]].copy_(torch.as_tensor(bvel, **kw))
    if p is not None:
        dom.pressure.copy_(torch.as_tensor(p, **kw))
    back = lambda t: t.cpu().numpy().astype(np.float64)
    return back(dom.velocity), back(dom.boundary_velocity), back(dom.pressure)


def random_fields(dom, rng, scale=1.0):
    d, N, NB = dom.dims, dom.n_cells, max(dom.n_boundary_faces, 1)
    return set_fields(dom, scale * rng.standard_normal((dom.batch, d, N)), scale * rng.standard_normal((dom.batch, d, NB)),
                      rng.standard_normal((dom.batch, N)))


def uniform_fields(dom, u):
    d, N, NB = dom.dims, dom.n_cells, max(dom.n_boundary_faces, 1)
    u = np.asarray(u, np.float64)
    return set_fields(dom, np.broadcast_to(u[None, :, None], (dom.batch, d, N)), np.broadcast_to(u[None, :, None], (dom.batch, d, NB)),
                      np.zeros((dom.batch, N)))


def face_centres(dom, ref):
    d = dom.dims
    bcell, bface, _ = dom.boundary_tables()
    return np.array([ref.X64[c, [k for k in range(1 << d) if ((k >> (f >> 1)) & 1) == (f & 1)]].mean(axis=0) for c, f in zip(bcell, bface)])


def path_bound(ref, calls, substeps, umax, h, G, T):
    """The fp32 bound of ``tests/test_gpu_tracers.py``: per sub-step the rounding of a position (4 eps L) and of a blended velocity
    (2 (2^d + 3) eps Umax h), amplified by exp(G T), times the safety factor 4."""
    return calls * substeps * (4 * EPS32 * ref.extent + 2 * ((1 << ref.dims) + 3) * EPS32 * umax * h) * np.exp(G * T) * 4


def to_dev(a, mesh, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(mesh.device, dtype)


# ------------------------------------------------------------------------------------------------ a: sampling
@pytest.mark.parametrize("prec", list(DTYPES))
@pytest.mark.parametrize("name", list(MESHES))
def test_sampling_matches_the_restatement(name, prec):
    dom, mesh, ref = case(name, prec)
    rng = np.random.default_rng(41)
    vel, bvel, p = random_fields(dom, rng)
    d = dom.dims
    cells = rng.integers(0, dom.n_cells, (B, N_PROBES)).astype(np.int32)
    xi = rng.random((B, N_PROBES, d))
    xi[:, :3] = np.round(xi[:, :3])                                   # corners and faces: w == 0 and w == 1
    xi_dev = to_dev(xi, mesh, dom.dtype)
    got = mesh.sample(to_dev(cells, mesh), xi_dev).cpu().numpy().astype(np.float64)
    F = max(np.abs(vel).max(), np.abs(p).max())
    K = max(ref.vel_w.shape[1], ref.cell_w.shape[1])
    tol = 1e-12 * F if prec == "fp64" else 4 * (K + 3 * d + 2) * EPS32 * ref.W * F
    xi_seen = xi_dev.cpu().numpy().astype(np.float64)
    for b in range(B):
        want = R.sample(ref, vel[b], bvel[b], [p[b]], cells[b], xi_seen[b])
        err = np.abs(got[b] - want).max()
        print(f"{name} {prec} env {b}: error {err:.3g}, bound {tol:.3g}")
        assert err <= tol
    # one point set for all envs, a field subset, a cell index outside the mesh (clamped before any load) and a NaN xi
    sub = mesh.sample(to_dev(cells[0], mesh), xi_dev[0], fields=("p", "u")).cpu().numpy().astype(np.float64)
    assert np.array_equal(sub[0], got[0][:, [d, 0]])
    wild = mesh.sample(to_dev(np.array([[-7, dom.n_cells + 5]] * B, np.int32), mesh),
                       to_dev(np.full((B, 2, d), np.nan), mesh, dom.dtype)).cpu().numpy()
    assert np.isfinite(wild).all()


# ------------------------------------------------------------------------------------------------ b: location
@pytest.mark.parametrize("prec", list(DTYPES))
@pytest.mark.parametrize("name", list(MESHES))
def test_location_gives_the_points_back(name, prec):
    dom, mesh, ref = case(name, prec)
    T = mesh.tables
    rng = np.random.default_rng(21)                                   # the points of tests/test_mb_tracers_host.py::test_location
    cells = rng.integers(0, T.n_cells, 4000)
    pts = M.cell_map(T.cell_xyz[cells], rng.random((4000, T.dims)))
    probes = M.MeshProbes(mesh, pts)                                  # strict: status 0 everywhere, or this raises
    assert int(probes.status.abs().max()) == 0
    seen = probes.points.cpu().numpy().astype(np.float64)
    cell, xi = probes.cell.cpu().numpy(), probes.xi.cpu().numpy().astype(np.float64)
    back = R.map_jac(ref.X[cell[0]], xi[0])[0]
    tol = 8 * float(np.finfo(DTYPES[prec][1]).eps) * np.abs(ref.X).max()
    err = np.abs(back - seen).max()
    print(f"{name} {prec}: location error {err:.3g}, bound {tol:.3g}")
    assert err <= tol
    assert np.array_equal(cell[0], cell[1]) and np.array_equal(xi[0], xi[1])


@pytest.mark.parametrize("prec", list(DTYPES))
def test_points_outside_the_fluid_and_a_nan(prec):
    dom, mesh, ref = case("cylinder_2d", prec)
    random_fields(dom, np.random.default_rng(5))
    bc = face_centres(dom, ref)
    body = []                                                         # the face centres of the cylinder's wall: their mean lies in the body
    for b, f in ((0, 1), (1, 2), (2, 0), (3, 3)):                     # (left +x, top -y, right -x, bottom +y: envs/cylinder_grid.py)
        blk = dom.blocks[b]
        body.append(bc[blk.boundary_slot0[f]: blk.boundary_slot0[f] + blk.face_cells(f)])
    inside_body = np.concatenate(body).mean(axis=0)
    beyond = mesh.tables.bounds[1] + 0.5
    pts = np.stack([inside_body, beyond, np.full(2, np.nan), ref.centres[7]])
    with pytest.raises(ValueError, match="point 0 of env 0"):
        M.MeshProbes(mesh, pts)
    probes = M.MeshProbes(mesh, pts, strict=False)
    st = probes.status.cpu().numpy()
    assert st[0].tolist()[:2] == [1, 1] and st[0, 2] != 0 and st[0, 3] == 0
    out = probes.sample().cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(probes.xi.cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------ c: solid-body rotation
@pytest.mark.parametrize("prec", list(DTYPES))
def test_solid_body_rotation_across_the_seams(prec):
    dom, mesh, ref = case("twisted_ring", prec)
    omega, calls, substeps, dt = 1.0, 5, 10, 0.5
    rot = lambda x: omega * np.stack([-x[:, 1], x[:, 0]])
    uniform_fields(dom, [0.0, 0.0])
    vel, bvel = rot(ref.X64.mean(axis=1)), rot(face_centres(dom, ref))
    set_fields(dom, np.broadcast_to(vel, (B,) + vel.shape), np.broadcast_to(bvel, (B,) + bvel.shape))
    rng = np.random.default_rng(7)
    r0, th0 = rng.uniform(0.8, 1.2, (B, N_TRACERS)), rng.uniform(0, 2 * np.pi, (B, N_TRACERS))
    cloud = M.MeshTracerCloud(mesh, N_TRACERS, positions=np.stack([r0 * np.cos(th0), r0 * np.sin(th0)], axis=-1), substeps=substeps)
    start = cloud.seed_positions.cpu().numpy().astype(np.float64)
    start_cell = cloud.cell.cpu().numpy().copy()
    for _ in range(calls):
        cloud.advect(dt)
    h = float(DTYPES[prec][1](dt) / DTYPES[prec][1](substeps))
    a, n = omega * h, calls * substeps
    angle, grow = n * np.arctan2(a, 1 - a * a / 2), (1 + a ** 4 / 4) ** (n / 2)
    assert angle > 2 * np.pi / 3 + 0.3                                # more than a block spans: every tracer crosses a seam
    c, s = np.cos(angle), np.sin(angle)
    want = grow * np.stack([c * start[..., 0] - s * start[..., 1], s * start[..., 0] + c * start[..., 1]], axis=-1)
    got = cloud.positions.cpu().numpy().astype(np.float64)
    T = calls * dt
    tol = 1e-11 * ref.extent if prec == "fp64" else path_bound(ref, calls, substeps, omega * 1.5, h, omega, T)
    err = np.abs(got - want).max()
    print(f"rotation {prec}: error {err:.3g}, bound {tol:.3g}")
    assert err <= tol
    assert int(cloud.lost.sum()) == 0 and (cloud.cell.cpu().numpy() != start_cell).all()
    assert np.allclose(cloud.age.cpu().numpy(), T) and np.array_equal(cloud.displacement().cpu().numpy(), (cloud.positions - cloud.seed_positions).cpu().numpy())


# ------------------------------------------------------------------------------------------------ d: walls, outflow, rotated seam
@pytest.mark.parametrize("prec", list(DTYPES))
def test_walls_outflow_and_the_rotated_seam(prec):
    dom, mesh, ref = case("split_rotated_channel", prec)
    uniform_fields(dom, [1.0, 0.0])
    rng = np.random.default_rng(9)
    seeds = np.stack([rng.uniform(0.2, 0.6, (B, N_TRACERS)), rng.uniform(0.2, 0.8, (B, N_TRACERS))], axis=-1)
    x_far = ref.X64[:, :, 0].max()
    loc = 8 * float(np.finfo(DTYPES[prec][1]).eps) * np.abs(ref.X).max()
    far = dom.blocks[1]                                               # (its -y face is the far end of the channel: the block is stored turned)
    slots = np.arange(far.boundary_slot0[2], far.boundary_slot0[2] + far.face_cells(2))
    free, flagged = M.MeshTracerCloud(mesh, N_TRACERS, positions=seeds), M.MeshTracerCloud(mesh, N_TRACERS, positions=seeds, respawn_slots=slots)
    start = free.seed_positions.cpu().numpy().astype(np.float64)
    calls, dt = 3, 0.5
    for _ in range(calls):
        free.advect(dt); flagged.advect(dt)
    h = float(DTYPES[prec][1](dt) / 4)
    tol = 1e-11 * ref.extent if prec == "fp64" else path_bound(ref, calls, 4, 1.0, h, 0.0, calls * dt)
    got = free.positions.cpu().numpy().astype(np.float64)
    assert np.abs(got - (start + [1.5, 0.0])).max() <= tol            # across the connection at the speed they had
    assert (free.cell.cpu().numpy() >= far.cell_offset).all() and np.array_equal(free.positions.cpu().numpy(), flagged.positions.cpu().numpy())
    reborn = np.zeros((B, N_TRACERS), bool)
    for _ in range(6):
        free.advect(dt); flagged.advect(dt)
        now = flagged.age.cpu().numpy() == 0
        assert np.array_equal(flagged.positions.cpu().numpy()[now], flagged.seed_positions.cpu().numpy()[now])
        assert np.array_equal(flagged.cell.cpu().numpy()[now], flagged.seed_cell.cpu().numpy()[now])
        reborn |= now
    assert reborn.all() and int(flagged.lost.sum()) == 0
    got = free.positions.cpu().numpy().astype(np.float64)
    assert np.abs(got[..., 0] - x_far).max() <= loc and np.abs(got[..., 1] - start[..., 1]).max() <= tol + loc      # on the far face
    free.advect(dt)
    again = free.positions.cpu().numpy().astype(np.float64)
    assert np.abs(again - got).max() <= loc and np.allclose(free.age.cpu().numpy(), 10 * dt) and int(free.lost.sum()) == 0
    # onto the lower wall, where they stop while their age keeps counting
    uniform_fields(dom, [0.0, -1.0])
    down = M.MeshTracerCloud(mesh, N_TRACERS, positions=np.stack([rng.uniform(0.2, 3.3, (B, N_TRACERS)), rng.uniform(0.2, 0.8, (B, N_TRACERS))], axis=-1))
    first = down.seed_positions.cpu().numpy().astype(np.float64)
    for _ in range(2):
        down.advect(0.5)
    got = down.positions.cpu().numpy().astype(np.float64)
    assert np.abs(got[..., 1]).max() <= loc and np.abs(got[..., 0] - first[..., 0]).max() <= tol + loc
    assert np.allclose(down.age.cpu().numpy(), 1.0) and int(down.lost.sum()) == 0


# ------------------------------------------------------------------------------------------------ e: periodic span
@pytest.mark.parametrize("prec", list(DTYPES))
def test_periodic_span(prec):
    dom, mesh, ref = case("skewed_pair_3d", prec)
    w, calls, dt = 0.7, 4, 0.5
    uniform_fields(dom, [0.0, 0.0, w])
    cloud = M.MeshTracerCloud(mesh, N_TRACERS, seed=3)
    z0 = cloud.seed_positions.cpu().numpy().astype(np.float64)[..., 2]
    for _ in range(calls):
        cloud.advect(dt)
    T = calls * dt
    Lz = float(np.abs(ref.shifts[0, 2]))
    h = float(DTYPES[prec][1](dt) / 4)
    tol = 1e-11 * ref.extent if prec == "fp64" else path_bound(ref, calls, 4, w, h, 0.0, T)
    un = cloud.unwrapped().cpu().numpy().astype(np.float64)
    err = np.abs(un[..., 2] - (z0 + w * T)).max()
    print(f"periodic {prec}: error {err:.3g}, bound {tol:.3g}")
    assert err <= tol
    sign = 1 if mesh.tables.shifts[0, 2] > 0 else -1
    assert np.array_equal(sign * cloud.wraps.cpu().numpy()[..., 0], np.floor((z0 + w * T - ref.X64[:, :, 2].min()) / Lz).astype(np.int64))
    pos = cloud.positions.cpu().numpy()
    assert (pos[..., 2] >= -tol).all() and (pos[..., 2] <= Lz + tol).all() and int(cloud.lost.sum()) == 0


# ------------------------------------------------------------------------------------------------ f: tracers against the restatement
SEED_F = 4          # the restatement alone keeps >= 80 % of these tracers 10 slack away from every face (checked on the CPU)


@pytest.mark.parametrize("prec", list(DTYPES))
@pytest.mark.parametrize("name", ["cylinder_2d", "cylinder_3d_small"])
def test_tracers_match_the_restatement(name, prec):
    dom, mesh, ref = case(name, prec)
    vel, bvel, _ = random_fields(dom, np.random.default_rng(17), scale=0.3)
    calls, substeps, dt = 3, 4, 0.05
    cloud = M.MeshTracerCloud(mesh, N_TRACERS, seed=SEED_F, substeps=substeps)
    state = {k: getattr(cloud, k).cpu().numpy() for k in ("positions", "cell", "age", "wraps", "seed_positions", "seed_cell")}
    for _ in range(calls):
        cloud.advect(dt)
    got, got_cell = cloud.positions.cpu().numpy().astype(np.float64), cloud.cell.cpu().numpy()
    respawn = np.zeros(max(dom.n_boundary_faces, 1), np.uint8)
    for b in range(B):
        x, c, age, wr = state["positions"][b].astype(np.float64), state["cell"][b], state["age"][b], state["wraps"][b]
        margin, lost = np.full(N_TRACERS, np.inf), 0
        for _ in range(calls):
            x, c, age, wr, l, m = R.advect(ref, vel[b], bvel[b], respawn, state["seed_positions"][b], state["seed_cell"][b], x, c, age, wr, dt, substeps)
            margin, lost = np.minimum(margin, m), lost + l
        if prec == "fp64":
            assert np.abs(got[b] - x).max() <= 1e-12 * ref.extent
            assert np.array_equal(got_cell[b], c) and int(cloud.lost[b]) == lost
            assert np.array_equal(cloud.wraps[b].cpu().numpy().reshape(N_TRACERS, -1), wr)
        else:
            keep = margin >= 10 * ref.slack
            assert keep.mean() >= 0.8
            vv = R.vertex_velocity(ref, vel[b], bvel[b])[ref.cell_vert]                       # [N, 2^d, d]
            G = ((vv.max(axis=1) - vv.min(axis=1)).max(axis=1) / ref.shortest).max()
            h = float(np.float32(dt) / np.float32(substeps))
            tol = path_bound(ref, calls, substeps, np.abs(vv).max(), h, G, calls * dt)
            err = np.abs(got[b] - x)[keep].max()
            print(f"{name} env {b}: {keep.sum()} tracers compared, error {err:.3g}, bound {tol:.3g}")
            assert err <= tol


# ------------------------------------------------------------------------------------------------ g: independence, repeatability
@pytest.mark.parametrize("prec", list(DTYPES))
def test_an_env_does_not_depend_on_the_batch_and_runs_repeat(prec):
    dom, mesh, ref = case("cylinder_3d_small", prec)
    vel, bvel, p = random_fields(dom, np.random.default_rng(23), scale=0.3)
    one, mesh1, _ = case("cylinder_3d_small", prec, batch=1)
    set_fields(one, vel[1:], bvel[1:], p[1:])
    pts = ref.centres[np.random.default_rng(2).integers(0, dom.n_cells, N_PROBES)] + 1e-3

    def run(m, env):
        cloud = M.MeshTracerCloud(m, N_TRACERS, seed=6)
        if m is mesh1:                                                # env 1's seeds: the draw of generator [seed, 1]
            full = M.MeshTracerCloud(mesh, N_TRACERS, seed=6)
            cloud.load_state_dict({**cloud.state_dict(), **{k: getattr(full, k)[1:2].clone() for k in ("positions", "seed_positions", "cell", "seed_cell")}})
        for _ in range(3):
            cloud.advect(0.05)
        probed = M.MeshProbes(m, pts).sample()
        return [t[env].cpu().numpy() for t in (cloud.positions, cloud.cell, cloud.age, cloud.wraps, probed, cloud.sample())]

    a, b, alone = run(mesh, 1), run(mesh, 1), run(mesh1, 0)
    for x, y, z in zip(a, b, alone):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    # state_dict -> load_state_dict -> advect replays bit for bit
    cloud = M.MeshTracerCloud(mesh, N_TRACERS, seed=6)
    cloud.advect(0.05)
    saved = cloud.state_dict()
    cloud.advect(0.05)
    want = [getattr(cloud, k).clone() for k in ("positions", "cell", "age", "wraps", "lost")]
    other = M.MeshTracerCloud(mesh, N_TRACERS, seed=99)
    other.load_state_dict(saved)
    other.advect(0.05)
    for k, t in zip(("positions", "cell", "age", "wraps", "lost"), want):
        assert torch.equal(getattr(other, k), t), k
    cloud.reseed([0])
    assert torch.equal(cloud.positions[0], cloud.seed_positions[0]) and torch.equal(cloud.positions[1], want[0][1]) and float(cloud.age[0].max()) == 0


# ------------------------------------------------------------------------------------------------ h: envs
def _cylinder():
    return fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=2, resolution=8, initial_domain_steps=6, randomize_initial_state=False,
                             step_length=0.05, dt=0.01, episode_length=3)


def _airfoil():
    return fluidgym_amd.make("Airfoil2D-easy-v0", num_envs=2, initial_domain_steps=6, randomize_initial_state=False, episode_length=3,
                             resolution_div=2)


@pytest.mark.parametrize("make", [_cylinder, _airfoil], ids=["cylinder", "airfoil"])
def test_env_probes_and_an_episode_with_tracers(make):
    env = make()
    obs0, _ = env.reset(seed=1)
    dom = env._domain
    ref = R.RefMesh(dom, np.float32)
    lo, hi = ref.X64.reshape(-1, 2).min(axis=0), ref.X64.reshape(-1, 2).max(axis=0)
    rake = np.stack([np.full(N_PROBES, lo[0] + 0.7 * (hi[0] - lo[0])), np.linspace(lo[1] + 0.1 * (hi[1] - lo[1]), hi[1] - 0.1 * (hi[1] - lo[1]), N_PROBES)], axis=-1)
    probes = env.locate_probes(rake)
    got = probes.sample().cpu().numpy().astype(np.float64)
    back = lambda t: t.cpu().numpy().astype(np.float64)
    vel, bvel, p = back(dom.velocity), back(dom.boundary_velocity), back(dom.pressure)
    cell, xi = probes.cell.cpu().numpy(), back(probes.xi)
    F = max(np.abs(vel).max(), np.abs(p).max())
    tol = 4 * (max(ref.vel_w.shape[1], ref.cell_w.shape[1]) + 3 * 2 + 2) * EPS32 * ref.W * F
    for b in range(2):
        assert np.abs(got[b] - R.sample(ref, vel[b], bvel[b], [p[b]], cell[b], xi[b])).max() <= tol
    assert np.abs(R.map_jac(ref.X[cell[0]], xi[0])[0] - back(probes.points)).max() <= 8 * EPS32 * np.abs(ref.X).max()
    # an episode with an active cloud computes what it computes without one
    actions = [env.sample_action() for _ in range(3)]
    plain = [env.step(a)[:2] for a in actions]
    env.reset(seed=1)
    cloud = env.start_mesh_tracers(N_TRACERS, seed=0, every=2)
    assert env.mesh_tracers is cloud and env.tracers is None
    with_cloud = [env.step(a)[:2] for a in actions]
    for (o1, r1), (o2, r2) in zip(plain, with_cloud):
        assert torch.equal(r1, r2)
        if isinstance(o1, dict):
            assert all(torch.equal(o1[k], o2[k]) for k in o1)
        else:
            assert torch.equal(o1, o2)
    assert float(cloud.age.max()) > 0 and np.isfinite(cloud.positions.cpu().numpy()).all()
    flagged = env._mesh_respawn_slots()
    assert flagged.any() and not flagged.all() and np.array_equal(cloud.respawn_slots.cpu().numpy()[:len(flagged)], flagged)
    state = env.get_state()
    assert "mesh_tracers" in state
    env.reset(seed=1)
    assert torch.equal(cloud.positions, cloud.seed_positions) and float(cloud.age.max()) == 0
    env.set_state(state)
    assert torch.equal(cloud.positions, state["mesh_tracers"]["cloud"]["positions"])
    assert env.stop_mesh_tracers() is cloud and env.mesh_tracers is None
    with pytest.raises(NotImplementedError, match="single-block"):
        env.probe(np.zeros((1, 2)))
    env.close()
    assert env._point_mesh is None
