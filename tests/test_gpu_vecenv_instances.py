"""GPU: DuckietownVecEnv(instance_shape=..., boxes=True) -- info["instances"] is the instance map (dtsim_instances) and info["boxes"] its
reduction (dtsim_boxes) of the state whose observation `obs` shows, byte for byte what the literal call sequence gives on a twin
BatchedSimulator; with final_obs=True info["final_instances"] / info["final_boxes"] hold, for the envs that finished a step, the rows before
the reset, and their rows of info["instances"] / info["boxes"] their new episode's first state; obs, reward, done and every other info entry
(depth and labels among them) are bit-identical to an env built without the new options; with label_shape == instance_shape one
dtsim_instances launch fills both maps and labels() is never called; without instance_shape neither new call is made.
64 x 48 cameras, N = 4 .. 6, max_steps = 3: every env finishes."""
import pytest

from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi

pytestmark = pytest.mark.gpu

STEPS, MAX_STEPS = 8, 3
CAM = dict(camera_width=64, camera_height=48)
MAP = "small_loop_only_duckies"
CONFIGS = {
    # N, obs_shape, instance_shape, boxes, env arguments (also given to the env without the new options), simulator arguments
    "plain": (4, (24, 32), (24, 32), True, dict(), dict(domain_rand=False)),
    "no_boxes_dr": (4, (24, 32), (48, 64), False, dict(), dict(domain_rand=True)),
    "final": (5, (24, 32), (48, 64), True, dict(final_obs=True), dict(domain_rand=False, distortion=True)),
    "final_no_boxes": (4, None, (12, 16), False, dict(final_obs=True), dict(domain_rand=False)),
    "depth": (4, (24, 32), (24, 32), True, dict(final_obs=True, depth_shape=(12, 16)), dict(domain_rand=False)),
    "labels_fused": (6, (24, 32), (24, 32), True, dict(final_obs=True, label_shape=(24, 32)), dict(domain_rand=False)),
    "labels_fused_plain": (4, (24, 32), (48, 64), True, dict(label_shape=(48, 64), depth_shape=(24, 32)), dict(domain_rand=False, distortion=True)),
    "labels_separate": (4, (24, 32), (24, 32), True, dict(final_obs=True, label_shape=(12, 16)), dict(domain_rand=False)),
    "stack": (4, (24, 32), (24, 32), True, dict(frame_stack=2), dict(domain_rand=False)),
    "stack_final": (4, (24, 32), (12, 16), True, dict(final_obs=True, frame_stack=2, grayscale=True), dict(domain_rand=False)),
}


class Tracer:
    """Counts, per simulator, the calls of BatchedSimulator.labels / instances / boxes, and the instances calls that carry a label map."""

    def __init__(self, monkeypatch):
        self.n = {}
        for name in ("labels", "instances", "boxes"):
            monkeypatch.setattr(BatchedSimulator, name, self._wrap(name, getattr(BatchedSimulator, name)))

    def _wrap(self, name, fn):
        def call(sim, *a, **k):
            n = self.n.setdefault(id(sim), dict(labels=0, instances=0, boxes=0, fused=0))
            n[name] += 1
            if name == "instances" and k.get("labels_out") is not None:
                n["fused"] += 1
            return fn(sim, *a, **k)
        return call

    def of(self, env):
        return self.n.get(id(env.sim), dict(labels=0, instances=0, boxes=0, fused=0))


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_instances_and_boxes_ride_with_the_observation(cfg, monkeypatch):
    import torch
    N, obs_shape, ishape, boxes, env_kw, sim_kw = CONFIGS[cfg]
    kw = dict(sim_kw, max_steps=MAX_STEPS, **CAM)
    A = DuckietownVecEnv(MAP, N, obs_shape=obs_shape, seed=4, instance_shape=ishape, boxes=boxes, **env_kw, **kw)
    B = DuckietownVecEnv(MAP, N, obs_shape=obs_shape, seed=4, **env_kw, **kw)
    ref = BatchedSimulator(MAP, N, action_mode="vel_steer", seed=4, device_reset=True, auto_reset=False, do_reset=False, **kw)
    final = bool(env_kw.get("final_obs"))
    new_keys = {"instances", "boxes", "final_instances", "final_boxes"}

    def ref_pass():
        ref.render()
        i = ref.instances(ishape[0], ishape[1])
        b = ref.boxes(i)
        ref.sync()
        return i.clone(), b.clone()

    def same(x, y):
        return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))

    tr = Tracer(monkeypatch)
    oa, ob = A.reset(), B.reset()
    fused, with_labels = env_kw.get("label_shape") == ishape, "label_shape" in env_kw
    assert tr.of(A) == dict(instances=1, boxes=int(boxes), fused=int(fused), labels=int(with_labels and not fused))
    assert tr.of(B) == dict(instances=0, boxes=0, fused=0, labels=int(with_labels))
    ref.reset()
    assert same(oa, ob) and B.instances is None and B.boxes is None
    assert A.instances.shape == (N, *ishape) and A.instances.dtype == torch.uint8
    assert (A.boxes.shape == (N, _ffi.MAX_OBJECTS, 5) and A.boxes.dtype == torch.int32) if boxes else A.boxes is None
    torch.cuda.synchronize()
    ri, rb = ref_pass()
    assert torch.equal(A.instances, ri) and (not boxes or torch.equal(A.boxes, rb))      # the first frames' maps: env.instances / env.boxes
    if "label_shape" in env_kw:
        assert torch.equal(A.labels, B.labels)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_done, n_new, n_seen = torch.zeros(N, device="cuda"), 0, int(A.instances.any())
    for t in range(STEPS):
        a = torch.rand((N, 2), device="cuda", generator=g) * 2 - 1
        oa, ra, da, ia = A.step(a)
        ob, rb_, db, ib = B.step(a)
        torch.cuda.synchronize()
        ref.step(a)                                          # by hand: step -> render -> instances -> boxes -> reset_done -> render -> ...
        before_i, before_b = ref_pass()
        ref_done = torch.as_tensor(ref.field_device(_ffi.FIELD_DONE), device="cuda").to(torch.bool).clone()
        ref.reset_done()
        after_i, after_b = ref_pass()
        # everything the env without the new options returns: bit-identical
        assert same(oa, ob) and same(ra, rb_) and same(da, db) and torch.equal(da, ref_done), (cfg, t)
        assert set(ia) - new_keys == set(ib) and not (set(ib) & new_keys), (cfg, sorted(ia), sorted(ib))
        for key in ib:
            if key in ("final_obs", "final_depth", "final_labels"):
                assert same(ia[key][da], ib[key][db]), (cfg, t, key)
            else:
                assert same(ia[key], ib[key]), (cfg, t, key)
        assert ia["instances"] is A.instances                # one persistent tensor
        assert torch.equal(ia["instances"], after_i), (cfg, t)               # byte for byte, the restarted envs' first frames included
        assert torch.equal(after_i[~da], before_i[~da])
        if boxes:
            assert ia["boxes"] is A.boxes and torch.equal(ia["boxes"], after_b), (cfg, t)
        else:
            assert "boxes" not in ia and "final_boxes" not in ia
        if final:
            assert same(ia["final_instances"][da], before_i[da]), (cfg, t, int(da.sum()))
            assert ia["final_instances"].shape == A.instances.shape
            if boxes:
                assert same(ia["final_boxes"][da], before_b[da]), (cfg, t)
                assert ia["final_boxes"].shape == A.boxes.shape and ia["final_boxes"].dtype == torch.int32
        else:
            assert "final_instances" not in ia and "final_boxes" not in ia
        n_new += int((after_i[da] != before_i[da]).flatten(1).any(dim=1).sum())
        n_seen += int(after_i.any())
        n_done += da.float()
    assert float(n_done.min()) >= 2, cfg                     # every env finished at least twice
    assert n_seen > 0, cfg                                   # a duckie was in view at some step
    n = tr.of(A)                                             # one launch for both maps where the shapes agree, else one each; boxes after every instance map
    assert n["instances"] > STEPS and n["boxes"] == (n["instances"] if boxes else 0), (cfg, n)
    assert n["fused"] == (n["instances"] if fused else 0) and n["labels"] == (n["instances"] if with_labels and not fused else 0), (cfg, n)
    assert tr.of(B)["instances"] == tr.of(B)["boxes"] == 0
    for e in (A, B):
        e.close()
    ref.close()


def test_default_arguments_make_no_new_call(monkeypatch):
    import torch
    tr = Tracer(monkeypatch)
    env = DuckietownVecEnv(MAP, 4, obs_shape=(24, 32), seed=4, final_obs=True, label_shape=(24, 32), depth_shape=(24, 32), max_steps=MAX_STEPS,
                           domain_rand=False, **CAM)
    env.reset()
    for _ in range(4):
        _, _, _, info = env.step(torch.zeros((4, 2), device="cuda"))
        assert not {"instances", "boxes", "final_instances", "final_boxes"} & set(info)
    torch.cuda.synchronize()
    assert tr.of(env)["instances"] == 0 and tr.of(env)["boxes"] == 0 and tr.of(env)["labels"] > 0
    assert env.instances is None and env.boxes is None
    env.close()
