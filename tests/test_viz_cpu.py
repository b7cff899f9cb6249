"""CPU (no GPU needed): what the image-grid test table is worth, the host restatement's own geometry, and the host side of
hr_viton_amd.viz -- BoardLog's files, ImageWriter, the scripts' new flags, the ``aux`` keywords."""
import inspect
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

import viz_cases as VC


def _viz():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import viz
    return viz


# ----------------------------------------------------------------------------------------- the table
def test_boundary_table_is_worth_its_name():
    tab = VC.boundary_table()
    assert tab.numel() == 3315 and tab.dtype == torch.float32
    prod = tab * 255                                             # fp32 product, rounded once
    frac = prod - prod.floor()
    half = frac == 0.5
    assert int(half.sum()) >= 250, int(half.sum())               # v * 255 lands exactly on k + 0.5
    rnd = VC.quant_round(tab.reshape(1, 1, -1).expand(3, -1, -1))[0, :, 0].to(torch.int64)
    trn = VC.quant_trunc(tab.reshape(1, 1, -1).expand(3, -1, -1).contiguous())[0, :, 0].to(torch.int64)
    even = torch.from_numpy(np.rint(prod.numpy())).to(torch.int64)      # round-half-even
    assert int((even != rnd).sum()) >= 100, int((even != rnd).sum())
    assert int((rnd != trn).sum()) >= 1500, int((rnd != trn).sum())


def test_the_three_signed_expressions_are_one_number():
    g = torch.Generator().manual_seed(0)
    for t in (VC.table_signed(VC.boundary_table()), torch.rand(1_000_000, generator=g) * 2.4 - 1.2):
        a, b, c = VC.signed_a(t), VC.signed_b(t), VC.signed_c(t)
        assert torch.equal(a, b) and torch.equal(a, c)
        # and so are the save_images bytes and the TRUNC bytes of the SIGNED value
        img = t[:999].reshape(1, 1, 999).expand(3, -1, -1).contiguous()
        assert np.array_equal(VC.save_images_array(img), VC.quant_trunc(VC.signed_a(img)).numpy())


def test_palette_round_trip():
    viz = _viz()
    assert viz.PALETTE == VC.PALETTE and len(VC.PALETTE) == 60
    p = torch.tensor(VC.PALETTE, dtype=torch.uint8)
    f = p.to(torch.float32).div(255)                             # ToTensor
    back_r = f.clone().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
    back_t = torch.from_numpy((f.numpy() * 255).clip(0, 255).astype(np.uint8))
    assert torch.equal(back_r, p) and torch.equal(back_t, p)
    # visualize_segmap's restatement shows class c in palette colour c
    x = torch.zeros(1, 20, 4, 5)
    for c in range(20):
        x[0, c, c // 5, c % 5] = 1.0
    rgb = (VC.ref_visualize_segmap(x) * 255).round().to(torch.uint8)
    for c in range(20):
        assert rgb[:, c // 5, c % 5].tolist() == VC.PALETTE[3 * c:3 * c + 3]


@pytest.mark.parametrize("n", [1, 2, 4, 5, 10, 12])
def test_restated_make_grid_shape_and_border(n):
    viz = _viz()
    H, W, p = 5, 7, 2
    imgs = [torch.full((3, H, W), float(k + 1)) for k in range(n)]
    g = VC.ref_make_grid(imgs, nrow=4, padding=p)
    assert tuple(g.shape[1:]) == VC.ref_shape(n, H, W, 4, p) == viz.grid_shape(n, H, W, 4, p)
    if n == 1:
        assert torch.equal(g, imgs[0])
        return
    xmaps = min(4, n)
    ymaps = -(-n // xmaps)
    assert g.shape[1] == ymaps * (H + p) + p and g.shape[2] == xmaps * (W + p) + p
    seen = torch.zeros_like(g[0], dtype=torch.bool)
    for k in range(n):
        y0, x0 = (k // xmaps) * (H + p) + p, (k % xmaps) * (W + p) + p
        assert (g[:, y0:y0 + H, x0:x0 + W] == k + 1).all()
        seen[y0:y0 + H, x0:x0 + W] = True
    assert (g[:, ~seen] == 0).all()                              # borders and the unfilled cells of the last row


# ----------------------------------------------------------------------------------------- BoardLog / ImageWriter
def _image(seed, H=9, W=7):
    return torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def test_board_log_file_layout_and_summary_writer(tmp_path, monkeypatch):
    viz = _viz()
    calls = []

    class SummaryWriter(object):
        def __init__(self, log_dir=None):
            calls.append(("init", log_dir))

        def add_scalar(self, tag, value, step):
            calls.append(("scalar", tag, value, step))

        def add_image(self, tag, img, step, dataformats="CHW"):
            calls.append(("image", tag, img, step, dataformats))

        def close(self):
            calls.append(("close",))

    stand_in = types.ModuleType("tensorboardX")
    stand_in.SummaryWriter = SummaryWriter
    monkeypatch.setitem(sys.modules, "tensorboardX", stand_in)
    d = str(tmp_path / "run")
    log = viz.BoardLog(d)
    a, b = _image(1), _image(2)
    log.add_image("train_images", a, 1)
    log.add_image("test_images/0", b.numpy(), 12)
    log.add_scalar("Loss/G", 0.5, 12)
    log.close()
    pa, pb = os.path.join(d, "images", "train_images", "00000001.png"), os.path.join(d, "images", "test_images_0", "00000012.png")
    assert os.path.isfile(pa) and os.path.isfile(pb)
    assert np.array_equal(np.asarray(Image.open(pa)), a.numpy()) and np.array_equal(np.asarray(Image.open(pb)), b.numpy())
    assert [c[0] for c in calls] == ["init", "image", "image", "scalar", "close"] and calls[0][1] == d
    for c, want, tag, step in ((calls[1], a, "train_images", 1), (calls[2], b, "test_images/0", 12)):
        assert c[1] == tag and c[3] == step and c[4] == "HWC"
        assert isinstance(c[2], np.ndarray) and c[2].dtype == np.uint8 and np.array_equal(c[2], want.numpy())
    with open(os.path.join(d, "scalars.jsonl")) as f:
        assert [json.loads(line) for line in f] == [{"tag": "Loss/G", "value": 0.5, "step": 12}]
    with pytest.raises(ValueError):
        log.add_image("x", torch.zeros(3, 4, 5), 1)


def test_board_log_without_a_summary_writer(tmp_path, monkeypatch):
    viz = _viz()
    from hr_viton_amd import validate
    monkeypatch.setattr(validate, "_summary_writer_class", lambda: None)
    log = viz.BoardLog(str(tmp_path / "r"))
    assert not (tmp_path / "r").exists()                        # nothing before the first record
    log.add_image("a/b/c", _image(3), 7)
    log.close()
    assert (tmp_path / "r" / "images" / "a_b_c" / "00000007.png").is_file() and not (tmp_path / "r" / "scalars.jsonl").exists()


def test_image_writer_threads_write_the_same_pixels(tmp_path):
    viz = _viz()
    imgs = [_image(10 + k, 33, 25) for k in range(7)]
    for workers in (0, 2):
        d = tmp_path / f"w{workers}"
        d.mkdir()
        with viz.ImageWriter(workers) as w:
            for k, im in enumerate(imgs):
                arr = im.numpy().copy()
                viz.save_image(arr, str(d / f"{k}.png"), w)
                arr[:] = 0                                       # the job owns its array: the caller may reuse its own
    for k, im in enumerate(imgs):
        a, b = np.asarray(Image.open(tmp_path / "w0" / f"{k}.png")), np.asarray(Image.open(tmp_path / "w2" / f"{k}.png"))
        assert np.array_equal(a, im.numpy()) and np.array_equal(a, b)
    with pytest.raises(ValueError):
        viz.ImageWriter(5)


def test_image_writer_close_reraises_a_workers_exception(tmp_path):
    viz = _viz()
    w = viz.ImageWriter(2)
    w.write(_image(1).numpy(), str(tmp_path / "ok.png"))
    w.write(_image(2).numpy(), str(tmp_path / "no_such_dir" / "x.png"))
    w.write(_image(3).numpy(), str(tmp_path / "ok2.png"))
    with pytest.raises(OSError):
        w.close()
    assert (tmp_path / "ok.png").is_file() and (tmp_path / "ok2.png").is_file()
    w.close()                                                   # a second close has nothing left to raise


def test_cpu_tensors_raise_and_unused_modes_are_not_implemented():
    viz = _viz()
    from hr_viton_amd.ops import HrvError
    with pytest.raises(HrvError):
        viz.Panel(torch.zeros(1, 3, 4, 4), viz.SIGNED)
    with pytest.raises(HrvError):
        viz.visualize_segmap(torch.zeros(1, 13, 4, 4))
    with pytest.raises(NotImplementedError):
        viz.visualize_segmap(torch.zeros(1, 13, 4, 4), multi_channel=False)
    with pytest.raises(NotImplementedError):
        viz.visualize_segmap(torch.zeros(1, 13, 4, 4), tensor_out=False)
    assert list(inspect.signature(viz.visualize_segmap).parameters) == ["input", "multi_channel", "tensor_out", "batch"]
    assert list(inspect.signature(viz.save_images).parameters)[:3] == ["img_tensors", "img_names", "save_dir"]


def test_entry_point_refuses_bad_arguments():
    import ctypes as C
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from hr_viton_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    assert C.sizeof(_lib.hrv_viz_panel_t) == 48
    p = (_lib.hrv_viz_panel_t * 1)()
    p[0].ptr, p[0].C, p[0].kind = 4096, 3, _lib.VIZ_SIGNED
    out = 8192

    def call(npanels=1, nrow=4, padding=2, N=1, H=4, W=4, quant=0, o=out):
        return lib.hrv_viz_grid_u8(p, npanels, nrow, padding, N, H, W, quant, o, None)

    assert call(npanels=0) == -1 and b"panels" in lib.hrv_last_error()
    assert call(npanels=17) == -1 and call(nrow=0) == -1 and call(padding=-1) == -1 and call(quant=2) == -1
    assert call(N=0) == -1 and call(o=None) == -1 and call(o=out + 1) == -1
    p[0].C = 2
    assert call() == -1
    p[0].C, p[0].kind = 21, _lib.VIZ_SEGMAP
    assert call() == -1 and b"SEGMAP" in lib.hrv_last_error()
    p[0].C, p[0].kind = 3, 5
    assert call() == -1
    p[0].kind, p[0].sy = _lib.VIZ_UNIT, -1
    assert call() == -1
    p[0].sy, p[0].ptr = 4, None
    assert call() == -1
    p[0].ptr = 4096
    assert call(N=1 << 14, H=1 << 10, W=1 << 10) == -1 and b"too large" in lib.hrv_last_error()


# ----------------------------------------------------------------------------------------- scripts and signatures
# every option of the two training scripts before ``--board`` existed, with its default (``get_opt([])`` / ``get_opt(['--name', 'x'])``)
TRAIN_CONDITION_DEFAULTS = {
    'name': 'test', 'gpu_ids': '', 'workers': 4, 'batch_size': 8, 'fp16': False, 'dataroot': './data/', 'datamode': 'train',
    'data_list': 'train_pairs.txt', 'fine_width': 192, 'fine_height': 256, 'tensorboard_dir': 'tensorboard',
    'checkpoint_dir': 'checkpoints', 'tocg_checkpoint': '', 'tensorboard_count': 100, 'display_count': 100, 'save_count': 10000,
    'load_step': 0, 'keep_step': 300000, 'shuffle': False, 'semantic_nc': 13, 'output_nc': 13, 'warp_feature': 'T1',
    'out_layer': 'relu', 'Ddownx2': False, 'Ddropout': False, 'num_D': 2, 'cuda': True, 'G_D_seperate': False, 'no_GAN_loss': False,
    'lasttvonly': False, 'interflowloss': False, 'clothmask_composition': 'warp_grad', 'edgeawaretv': 'no_edge', 'add_lasttv': False,
    'no_test_visualize': False, 'num_test_visualize': 3, 'test_datasetting': 'unpaired', 'test_dataroot': './data/',
    'test_data_list': 'test_pairs.txt', 'G_lr': 0.0002, 'D_lr': 0.0002, 'CElamda': 10, 'GANlambda': 1, 'tvlambda': 2,
    'upsample': 'bilinear', 'val_count': 1000, 'spectral': False, 'occlusion': False, 'synthetic': False, 'max_steps': 0, 'ngf': 96,
    'no_vgg_loss': False, 'vgg_weights': '', 'vgg_random_init': False, 'val_items': 2000}
TRAIN_GENERATOR_DEFAULTS = {
    'name': 'x', 'gpu_ids': [0], 'workers': 4, 'batch_size': 8, 'fp16': False, 'cuda': True, 'dataroot': './data/',
    'datamode': 'train', 'data_list': 'train_pairs.txt', 'fine_width': 768, 'fine_height': 1024, 'radius': 20, 'grid_size': 5,
    'tensorboard_dir': 'tensorboard', 'checkpoint_dir': 'checkpoints', 'tocg_checkpoint': None, 'gen_checkpoint': '',
    'dis_checkpoint': '', 'tensorboard_count': 100, 'display_count': 100, 'save_count': 10000, 'load_step': 0, 'keep_step': 100000,
    'decay_step': 100000, 'shuffle': False, 'lpips_count': 1000, 'test_datasetting': 'paired', 'test_dataroot': './data/',
    'test_data_list': 'test_pairs.txt', 'G_lr': 0.0001, 'D_lr': 0.0004, 'GMM_const': None, 'semantic_nc': 13, 'gen_semantic_nc': 7,
    'norm_G': 'spectralaliasinstance', 'norm_D': 'spectralinstance', 'ngf': 64, 'ndf': 64, 'num_upsampling_layers': 'most',
    'init_type': 'xavier', 'init_variance': 0.02, 'no_ganFeat_loss': False, 'no_vgg_loss': False, 'lambda_l1': 1.0,
    'lambda_feat': 10.0, 'lambda_vgg': 10.0, 'n_layers_D': 3, 'netD_subarch': 'n_layer', 'num_D': 2, 'GT': False, 'occlusion': False,
    'warp_feature': 'T1', 'out_layer': 'relu', 'clothmask_composition': 'warp_grad', 'num_test_visualize': 3, 'synthetic': False,
    'max_steps': 0, 'tocg_ngf': 96, 'vgg_weights': '', 'vgg_random_init': False,
    'lpips_weights': './eval_models/weights/v0.1/alex.pth', 'alexnet_weights': None, 'lpips_random_init': False, 'val_items': 500,
    'val_batch_size': 1}


def test_board_defaults_to_off_and_every_other_option_is_what_it_was():
    import train_condition as tc
    import train_generator as tg
    for mod, argv, want in ((tc, [], TRAIN_CONDITION_DEFAULTS), (tg, ["--name", "x"], TRAIN_GENERATOR_DEFAULTS)):
        assert vars(mod.get_opt(argv)) == dict(want, board=False)
        assert vars(mod.get_opt(argv + ["--board"])) == dict(want, board=True)


def test_write_grids_splits_its_flags_from_the_test_scripts():
    """write_grids.py takes --grid_dir / --image_workers / --with_outputs itself and hands every other flag to the get_opt of
    test_generator.py / test_condition.py, which are unchanged and know no such flag."""
    import test_condition as tcd
    import test_generator as tgn
    import write_grids as wg
    own, rest = wg.get_opt(["generator", "--grid_dir", "g", "--synthetic", "3", "-b", "2", "--ngf", "8"])
    assert (own.which, own.grid_dir, own.image_workers, own.with_outputs) == ("generator", "g", 0, False)
    assert rest == ["--synthetic", "3", "-b", "2", "--ngf", "8"]
    o = tgn.get_opt(rest)
    assert (o.synthetic, o.batch_size, o.ngf) == (3, 2, 8) and not hasattr(o, "grid_dir")
    own, rest = wg.get_opt(["condition", "--synthetic", "--image_workers", "2", "--grid_dir", "d", "--with_outputs"])
    assert (own.which, own.grid_dir, own.image_workers, own.with_outputs) == ("condition", "d", 2, True) and rest == ["--synthetic"]
    assert tcd.get_opt(rest).synthetic is True and not hasattr(tcd.get_opt([]), "grid_dir")
    with pytest.raises(SystemExit):
        wg.get_opt(["generator"])                                 # --grid_dir is what the tool is for
    with pytest.raises(SystemExit):
        tgn.get_opt(["--grid_dir", "g"])


def test_aux_keywords_default_to_none():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import pipeline
    for fn in (pipeline.condition_train_step, pipeline.make_generator_inputs, pipeline.generator_train_step):
        p = inspect.signature(fn).parameters["aux"]
        assert p.default is None


def test_docstrings_say_what_is_opt_in():
    import train_condition as tc
    import train_generator as tg
    import write_grids as wg
    viz = _viz()
    assert "--grid_dir" in wg.__doc__ and "generator/grid" in wg.__doc__ and "--with_outputs" in wg.__doc__
    assert "--board" in tc.__doc__ and "Loss/G/l1_cloth" in tc.__doc__ and "--board" in tg.__doc__ and "Loss/gen/feat" in tg.__doc__
    for phrase in ("first", "rank 0", "misalign", "TRUNC", "ROUND"):
        assert phrase in viz.__doc__, phrase
