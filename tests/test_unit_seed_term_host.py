"""Host: the one autograd Function of the one-pass loss terms (drt_amd.diffrender._UnitSeedTerm) driven by CPU tensors.

The terms are the ones the ``Scene`` methods build (``_ray_term``, ``_paths_ior_term``, ``_image_term`` at its three entry points,
``_image_views_term``) on a stand-in scene that only has vertices, with their ``enqueue`` replaced by one that writes fixed numbers into
whatever accumulators it is handed and records which those were.  Float64 mode is pinned (the deterministic mode converts its cells on
the device).  5 vertices; a 4 x 5 one-channel texture: 20 texels in an accumulator padded to 21, so the slice matters."""
import types

import numpy as np
import pytest
import torch

from drt_amd import _lib, det, diffrender as Render

N_V, TEX = 5, (4, 5)
FACTOR = 2.5                 # the downstream factor: loss * FACTOR is what backward() is called on
LOSS = 3.25


@pytest.fixture(autouse=True)
def _host_mode(monkeypatch):
    monkeypatch.setattr(det, "_state", [False])
    monkeypatch.setattr(Render, "_f64c", lambda t, name: t.contiguous())        # (the real one refuses CPU tensors)
    assert det.SINK is None


def _fixed(name, n):
    """The numbers the stand-in enqueue leaves in accumulator ``name``: distinct, none of them zero."""
    return (torch.arange(n, dtype=torch.float64) + 1.0) * {"vertices": 0.5, "ior": -3.0, "screen": 0.25, "texture": 7.0, "camera": -0.125}[name]


def _with_fake(term):
    seen = {}

    def enqueue(loss, cells):
        seen["cells"] = dict(cells)
        loss.fill_(LOSS)
        for name, c in cells.items():
            c.copy_(_fixed(name, c.numel()).reshape(c.shape))
    return term._replace(enqueue=enqueue), seen


def _scene(requires_grad=True):
    return types.SimpleNamespace(vertices=torch.linspace(0, 1, N_V * 3, dtype=torch.float64).reshape(N_V, 3).requires_grad_(requires_grad))


def _image_args(vertices=True, want_image=False):
    return dict(vertices=vertices, want_image=want_image, height=2, width=3, channels=1)


def _leaf(*shape, dtype=torch.float64, requires_grad=True):
    return torch.ones(shape, dtype=dtype).requires_grad_(requires_grad)


def _run(term, *inputs):
    term, seen = _with_fake(term)
    loss = Render._UnitSeedTerm.apply(term, *inputs)
    return loss, seen


# ------------------------------------------------------------------------------------------------------------------------- the gradients
@pytest.mark.parametrize("rows", [4, 3])
def test_every_gradient_is_stored_times_the_factor_in_its_inputs_own_form(rows):
    scene = _scene()
    ii, ie, P, T = _leaf(), _leaf(), _leaf(3, 3), _leaf(*TEX, dtype=torch.float32)
    Rinv, Kinv = _leaf(rows, 4), _leaf(3, 3)
    term = Render._image_term(scene, _image_args(), (1.5, 1.0), torch.zeros(TEX + (1,), dtype=torch.float32), None, None, "camera")
    loss, seen = _run(term, scene.vertices, ii, ie, P, T, Rinv, Kinv)
    assert loss.shape == () and loss.dtype == torch.float64 and float(loss.detach()) == LOSS
    assert set(seen["cells"]) == {"vertices", "ior", "screen", "texture", "camera"}
    assert seen["cells"]["texture"].numel() == 21 and seen["cells"]["camera"].numel() == 21 and seen["cells"]["screen"].numel() == 9
    (loss * FACTOR).backward()
    V = scene.vertices
    assert torch.equal(V.grad, (_fixed("vertices", N_V * 3) * FACTOR).reshape(N_V, 3)) and V.grad.dtype == torch.float64
    for k, x in enumerate((ii, ie)):
        assert x.grad.shape == () and x.grad.dtype == torch.float64 and x.grad.device == x.device
        assert torch.equal(x.grad, _fixed("ior", 2)[k] * FACTOR)
    assert P.grad.shape == (3, 3) and torch.equal(P.grad, (_fixed("screen", 9) * FACTOR).reshape(3, 3))
    assert T.grad.shape == TEX and T.grad.dtype == torch.float32
    assert torch.equal(T.grad, (_fixed("texture", 21)[:20] * FACTOR).reshape(TEX).to(torch.float32))
    cam = _fixed("camera", 21) * FACTOR
    assert Kinv.grad.shape == (3, 3) and torch.equal(Kinv.grad, cam[:9].reshape(3, 3))
    assert Rinv.grad.shape == (rows, 4) and Rinv.grad.dtype == torch.float64 and torch.equal(Rinv.grad[:3], cam[9:].reshape(3, 4))
    if rows == 4:
        assert not Rinv.grad[3].any()


def test_an_input_that_needs_no_gradient_gets_none():
    scene = _scene()
    ii, ie = _leaf(), _leaf(requires_grad=False)
    P, T = _leaf(3, 3, requires_grad=False), _leaf(*TEX)
    term = Render._image_term(scene, _image_args(), (1.5, 1.0), torch.zeros(TEX + (1,), dtype=torch.float32), None, None, "camera")
    loss, seen = _run(term, scene.vertices, ii, ie, P, T, None, _leaf(3, 3, requires_grad=False))
    assert set(seen["cells"]) == {"vertices", "ior", "texture"}           # no screen, no camera accumulator
    (loss * FACTOR).backward()
    assert ie.grad is None and P.grad is None
    assert torch.equal(ii.grad, _fixed("ior", 2)[0] * FACTOR) and T.grad is not None and scene.vertices.grad is not None


def test_without_vertices_there_is_no_vertex_accumulator_and_no_vertex_gradient():
    tex = torch.zeros(TEX + (1,), dtype=torch.float32)
    for build in (lambda s: Render._image_term(s, _image_args(vertices=False), (1.5, 1.0), tex, None, None, "plain"),
                  lambda s: Render._image_views_term(s, None, _image_args(vertices=False), (1.5, 1.0), tex, (2, "drop", "reference")),
                  lambda s: Render._paths_ior_term(s, None, None, None, None, (1.5, 1.0), 4, 1, False)):
        scene, ii = _scene(), _leaf()
        loss, seen = _run(build(scene), scene.vertices.detach(), ii, None)
        assert set(seen["cells"]) == {"ior"}
        (loss * FACTOR).backward()
        assert scene.vertices.grad is None and torch.equal(ii.grad, _fixed("ior", 2)[0] * FACTOR)
    # ... and a vertex input that is tracked all the same still receives nothing: there is nothing stored for it
    scene, ii = _scene(), _leaf()
    loss, _ = _run(Render._image_term(scene, _image_args(vertices=False), (1.5, 1.0), tex, None, None, "plain"), scene.vertices, ii, None)
    (loss * FACTOR).backward()
    assert scene.vertices.grad is None


# ------------------------------------------------------------------------------------------------------- each route's allocation rule
def test_the_ray_routes_always_have_a_vertex_accumulator_and_a_count_only_under_a_law():
    for law in (None, (4, "reflect", "reference")):
        scene = _scene()
        term = Render._ray_term(scene, None, None, None, None, (1.5, 1.0), law, None)
        assert (term.count is None) == (law is None) and term.image is None
        loss, seen = _run(term, scene.vertices)
        assert set(seen["cells"]) == {"vertices"} and seen["cells"]["vertices"].shape == (N_V, 3)
        (loss * FACTOR).backward()
        assert torch.equal(scene.vertices.grad, (_fixed("vertices", N_V * 3) * FACTOR).reshape(N_V, 3))
    scene = _scene(requires_grad=False)                      # nothing tracked: the accumulator is there all the same
    _, seen = _run(Render._ray_term(scene, None, None, None, None, (1.5, 1.0), None, None), scene.vertices)
    assert set(seen["cells"]) == {"vertices"}


def test_the_ior_pair_is_always_there_except_on_the_camera_route():
    """paths-IOR, image, image-screen and views: allocated with plain float IORs too; camera: only when an IOR input needs a gradient.
    Screen, texture and camera accumulators: only when that input is given and needs one."""
    tex = torch.zeros(TEX + (1,), dtype=torch.float32)
    a = _image_args()
    three = {"paths-ior": lambda s: Render._paths_ior_term(s, None, None, None, None, (1.5, 1.0), 4, 1, True),
             "image": lambda s: Render._image_term(s, a, (1.5, 1.0), tex, None, None, "plain"),
             "views": lambda s: Render._image_views_term(s, None, a, (1.5, 1.0), tex, (2, "drop", "reference"))}
    for name, build in three.items():
        scene = _scene()
        term = build(scene)
        assert term.count is not None and term.count.dtype == torch.int64 and term.count.shape == (), name
        _, seen = _run(term, scene.vertices, None, None)
        assert set(seen["cells"]) == {"vertices", "ior"}, name
    scene = _scene()
    screen = lambda: Render._image_term(scene, a, (1.5, 1.0), tex, None, None, "screen")      # noqa: E731
    camera = lambda: Render._image_term(scene, a, (1.5, 1.0), tex, None, None, "camera")      # noqa: E731
    V = scene.vertices
    assert set(_run(screen(), V, None, None, None, None)[1]["cells"]) == {"vertices", "ior"}
    assert set(_run(screen(), V, None, None, _leaf(3, 3), None)[1]["cells"]) == {"vertices", "ior", "screen"}
    assert set(_run(screen(), V, None, None, _leaf(3, 3, requires_grad=False), _leaf(*TEX))[1]["cells"]) == {"vertices", "ior", "texture"}
    assert set(_run(camera(), V, None, None, None, None, None, None)[1]["cells"]) == {"vertices"}
    assert set(_run(camera(), V, None, _leaf(), None, None, None, None)[1]["cells"]) == {"vertices", "ior"}
    assert set(_run(camera(), V, _leaf(requires_grad=False), None, None, None, _leaf(4, 4), None)[1]["cells"]) == {"vertices", "camera"}
    assert set(_run(camera(), V, None, None, None, None, _leaf(4, 4, requires_grad=False), _leaf(3, 3))[1]["cells"]) == {"vertices", "camera"}
    assert set(_run(camera(), V, None, None, None, None, _leaf(4, 4, requires_grad=False), None)[1]["cells"]) == {"vertices"}


def test_the_image_is_published_only_when_asked_for():
    scene, tex = _scene(), torch.zeros(TEX + (1,), dtype=torch.float32)
    assert Render._image_term(scene, _image_args(), (1.5, 1.0), tex, None, None).image is None
    image = Render._image_term(scene, _image_args(want_image=True), (1.5, 1.0), tex, None, None).image
    assert image.shape == (2, 3, 1) and image.dtype == torch.float32


# ------------------------------------------------------------------------------------------------------------------ enqueue_image_term
class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("drt_render_image_loss"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


def _enqueue(monkeypatch, **kw):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(Render, "_stream", lambda: 77)
    a = dict(height=4, width=3, channels=1, bands=[(0, 2), (2, 4)], supersample=1, max_bounces=2, law_flags=0, fresnel=1, camera=np.zeros(21),
             screen=np.zeros(9), void=np.zeros(1), invalid=np.zeros(1))
    scene = types.SimpleNamespace(optix_mesh=types.SimpleNamespace(_h=5))
    t = torch.zeros(4)
    Render.enqueue_image_term(scene, t, a, (1.5, 1.0), torch.zeros(TEX + (1,)), t, None, 11, 12, 13, None, 14, **kw)
    return fake.calls


@pytest.mark.parametrize("kw,name", [({}, "drt_render_image_loss"), ({"screen_ptr": 21}, "drt_render_image_loss_screen"),
                                     ({"texture_ptr": 22}, "drt_render_image_loss_screen"), ({"camera_ptr": 23}, "drt_render_image_loss_camera"),
                                     ({"entry": "screen"}, "drt_render_image_loss_screen"), ({"entry": "camera"}, "drt_render_image_loss_camera"),
                                     ({"texture_ptr": 22, "entry": "camera"}, "drt_render_image_loss_camera")])
def test_enqueue_image_term_takes_the_narrowest_entry_point_or_the_one_named(monkeypatch, kw, name):
    calls = _enqueue(monkeypatch, **kw)
    assert [c[0] for c in calls] == [name, name] and [c[1][5:7] for c in calls] == [(0, 2), (2, 4)]
    for _, args in calls:
        assert len(args) == len(_lib.SIGNATURES[name][1]) and args[-1] == 77
        assert args[22:27] == (11, 12, 13, None, 14)
        assert args[27:-1] == (kw.get("screen_ptr"), kw.get("texture_ptr"), kw.get("camera_ptr"))[:len(args) - 28]


def test_enqueue_image_term_refuses_an_entry_point_too_narrow(monkeypatch):
    for kw in ({"screen_ptr": 21, "entry": "plain"}, {"camera_ptr": 23, "entry": "screen"}):
        with pytest.raises(ValueError, match="has no parameter"):
            _enqueue(monkeypatch, **kw)
