"""GPU: csrc/viz.hip and hr_viton_amd.viz against the host restatement of the reference's chain (viz_cases.py).  Every comparison
is ``torch.equal``: the grids are bytes."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn as nn
from PIL import Image

import viz_cases as VC

pytestmark = pytest.mark.gpu


def _viz():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import viz
    return viz


def _act(t_nchw, cstride, pad_value=0.0):
    """An NHWC Act over a [N,H,W,cstride] tensor holding ``t_nchw``'s channels; the padding channels hold ``pad_value``."""
    from hr_viton_amd.ops import Act
    N, C, H, W = t_nchw.shape
    buf = torch.full((N, H, W, cstride), pad_value, dtype=torch.float32)
    buf[..., :C] = t_nchw.permute(0, 2, 3, 1)
    return Act(buf.cuda(), C)


def _panel(viz, how, t):
    kind = {"signed_a": viz.SIGNED, "signed_b": viz.SIGNED, "unit": viz.UNIT, "mask": viz.UNIT, "seg": viz.SEGMAP}[how]
    return viz.Panel(t.cuda(), kind)


# ----------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("H,W", VC.SIZES)
def test_grid_u8_equals_the_restatement(H, W):
    """Every (N, panel count, nrow, padding, quant) of the case table at one panel size; the panels cycle through the kinds and carry
    the boundary table (as far as the size holds it) plus values beyond both clamps."""
    viz = _viz()
    for N in VC.BATCHES:
        specs_all = VC.kind_cycle(12, N, H, W, seed=H * 100 + N)
        dev_all = [_panel(viz, how, t) for how, t in specs_all]
        for n, nrow in VC.COUNTS:
            for pad in VC.PADDINGS:
                for quant, q in ((VC.ROUND, viz.ROUND), (VC.TRUNC, viz.TRUNC)):
                    got = viz.grid_u8(dev_all[:n], nrow=nrow, padding=pad, quant=q)
                    want = VC.ref_grids(specs_all[:n], N, nrow, pad, quant)
                    assert got.dtype == torch.uint8 and tuple(got.shape) == (N,) + VC.ref_shape(n, H, W, nrow, pad) + (3,)
                    assert torch.equal(got.cpu(), want), (N, n, nrow, pad, quant)


@pytest.mark.parametrize("how", ["signed_a", "signed_b", "unit", "mask", "seg"])
def test_each_kind_alone_over_the_whole_boundary_table(how):
    """One kind in every panel; 33x25 + 64x48 hold the 3315 table values (and their 2v - 1 for SIGNED) several times over."""
    viz = _viz()
    for (H, W), n in (((33, 25), 5), ((64, 48), 2)):
        specs = []
        for k in range(n):
            if how == "seg":
                t = VC.seg_scores(2, 13 if k % 2 == 0 else 7, H, W, 50 + k)
            else:
                t = VC.fill((2, 1 if how == "mask" else 3, H, W), 60 + k, signed=how.startswith("signed"))
            specs.append((how, t))
        if how != "seg" and (H, W) == (64, 48):
            tab = VC.boundary_table()
            tab = VC.table_signed(tab) if how.startswith("signed") else tab
            flat = specs[0][1].view(-1)                           # panel 0 carries the whole table, in order
            assert flat.numel() >= tab.numel()
            flat[:tab.numel()] = tab
        dev = [_panel(viz, h, t) for h, t in specs]
        for quant, q in ((VC.ROUND, viz.ROUND), (VC.TRUNC, viz.TRUNC)):
            assert torch.equal(viz.grid_u8(dev, quant=q).cpu(), VC.ref_grids(specs, 2, 4, 2, quant)), (H, W, quant)


def test_round_is_two_step_and_not_half_even_on_the_device():
    """The table's half-integer products: the bytes are floor(fl(fl(v * 255) + 0.5)), checked value by value."""
    viz = _viz()
    tab = VC.boundary_table()
    img = torch.zeros(1, 3, 64, 48)
    img.view(-1)[:tab.numel()] = tab
    got = viz.grid_u8([viz.Panel(img.cuda(), viz.UNIT)], quant=viz.ROUND).cpu()       # [1,64,48,3]
    got_flat = got[0].permute(2, 0, 1).reshape(-1)[:tab.numel()].to(torch.int64)
    want = (tab * 255 + 0.5).clamp(0, 255).to(torch.uint8).to(torch.int64)            # two fp32 roundings
    assert torch.equal(got_flat, want)
    even = torch.from_numpy(np.rint((tab * 255).numpy())).to(torch.int64)
    assert int((got_flat != even).sum()) >= 100
    trunc = viz.grid_u8([viz.Panel(img.cuda(), viz.UNIT)], quant=viz.TRUNC).cpu()[0].permute(2, 0, 1).reshape(-1)[:tab.numel()]
    assert torch.equal(trunc.to(torch.int64), (tab * 255).clamp(0, 255).to(torch.uint8).to(torch.int64))
    assert int((trunc.to(torch.int64) != got_flat).sum()) >= 1500


def test_source_layouts_in_one_grid():
    """Contiguous NCHW, the slice [:, 6:9] of a 9-channel tensor, NHWC Acts (cstride 16 / 13 real as a segmentation map, cstride 4 /
    3 real as a colour image), an expanded mask (channel stride 0), a one-channel mask and a sample-0 panel, side by side -- no copy
    on the way in."""
    viz = _viz()
    from hr_viton_amd.ops import Act
    N, H, W = 3, 33, 25
    x9 = VC.fill((N, 9, H, W), 1, True)
    plain = VC.fill((N, 3, H, W), 2, True)
    seg13 = VC.seg_scores(N, 13, H, W, 3)
    col3 = VC.fill((N, 3, H, W), 4, False)
    mask = (VC.fill((N, 1, H, W), 5, False) > 0.3).float()
    first = VC.fill((N, 3, H, W), 6, True)
    seg7 = VC.seg_scores(N, 7, H, W, 7)
    x9d, maskd, firstd = x9.cuda(), mask.cuda(), first.cuda()
    a13, a3, a7 = _act(seg13, 16, pad_value=1e9), _act(col3, 4, pad_value=-7.0), _act(seg7, 8, pad_value=1e9)
    wide = torch.full((N, H, W, 24), 1e9)
    wide[..., 8:15] = seg7.permute(0, 2, 3, 1)
    a7_slice = Act(wide.cuda(), 7, 8)                                               # channels 8..14 of a wider NHWC tensor
    sl = x9d[:, 6:9]
    assert not sl.is_contiguous() and sl.data_ptr() != x9d.data_ptr()
    exp = maskd.expand(-1, 3, -1, -1)
    assert exp.stride(1) == 0
    panels = [viz.Panel(plain.cuda(), viz.SIGNED), viz.Panel(sl, viz.SIGNED), viz.Panel(a13, viz.SEGMAP), viz.Panel(a3, viz.UNIT),
              viz.Panel(exp, viz.UNIT), viz.Panel(maskd, viz.UNIT), viz.Panel(firstd[:1], viz.SIGNED), viz.Panel(a7, viz.SEGMAP),
              viz.Panel(a7_slice, viz.SEGMAP), viz.Panel(firstd[:1].expand(N, -1, -1, -1), viz.SIGNED)]
    assert panels[6].sn == 0 and panels[9].sn == 0 and panels[4].sc == 0 and panels[2].sx == 16 and panels[3].sx == 4
    specs = [("signed_a", plain), ("signed_a", x9[:, 6:9]), ("seg", seg13), ("unit", col3), ("mask", mask), ("mask", mask),
             ("signed_a", first[:1]), ("seg", seg7), ("seg", seg7), ("signed_a", first[:1])]
    for quant, q in ((VC.ROUND, viz.ROUND), (VC.TRUNC, viz.TRUNC)):
        got = viz.grid_u8(panels, quant=q)
        assert torch.equal(got.cpu(), VC.ref_grids(specs, N, 4, 2, quant))
    # the sources are untouched
    assert torch.equal(x9d.cpu(), x9) and torch.equal(a13.t[..., 13:].cpu(), torch.full((N, H, W, 3), 1e9))
    # count: the first grids only
    assert torch.equal(viz.grid_u8(panels, count=1).cpu(), VC.ref_grids(specs, 1, 4, 2, VC.ROUND))


@pytest.mark.parametrize("C,cstride", [(13, 16), (7, 8)])
def test_segmap_ties_and_padding_channels(C, cstride):
    """First maximum wins, like np.argmax: two equal maxima, all channels equal (index 0), +0.0 against -0.0; a maximum in the last
    real channel with a larger value planted in a padding channel of the Act, which must be ignored.  NCHW planes and NHWC float4
    groups read the same scores."""
    viz = _viz()
    H, W = 5, 7
    g = torch.Generator().manual_seed(C)
    x = torch.randn(1, C, H, W, generator=g)
    x[0, :, 0, 0] = 0.0
    x[0, 2, 0, 0] = x[0, C - 2, 0, 0] = 3.0                                         # two equal maxima -> 2
    x[0, :, 0, 1] = 1.5                                                             # all equal -> 0
    x[0, :, 0, 2] = -1.0
    x[0, 1, 0, 2], x[0, 4, 0, 2] = -0.0, 0.0                                        # -0.0 first, +0.0 later: equal -> 1
    x[0, :, 0, 3] = -1.0
    x[0, 1, 0, 3], x[0, 4, 0, 3] = 0.0, -0.0                                        # +0.0 first -> 1
    x[0, :, 0, 4] = -2.0
    x[0, C - 1, 0, 4] = 5.0                                                         # the last real channel
    x[0, :, 0, 5] = -5.0                                                            # all equal and negative -> 0 (padding is larger)
    x[0, :, 1, :] = torch.arange(W).float()[None, :].expand(C, -1)                  # all equal per pixel -> 0
    x[0, C - 1, 1, :] += 0.5                                                        # ... but for the last channel
    idx = np.argmax(x[0].numpy(), axis=0)
    assert idx[0, 0] == 2 and idx[0, 1] == 0 and idx[0, 2] == 1 and idx[0, 3] == 1 and idx[0, 4] == C - 1 and idx[0, 5] == 0
    assert (idx[1] == C - 1).all()
    want = VC.ref_grids([("seg", x)], 1, 4, 2, VC.ROUND)
    act = _act(x, cstride, pad_value=1e9)                                           # larger than every score
    assert float(act.t[..., C:].min()) == 1e9
    for src in (x.cuda(), act, x.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)):   # NCHW, Act, dense channels-last
        for q in (viz.ROUND, viz.TRUNC):
            assert torch.equal(viz.grid_u8([viz.Panel(src, viz.SEGMAP)], quant=q).cpu(), want)
    pal = torch.tensor(VC.PALETTE, dtype=torch.uint8).view(20, 3)
    assert torch.equal(want[0], pal[torch.from_numpy(idx)])


def test_grid_of_more_than_one_block_and_an_unaligned_tail():
    """1 x 1, 1 x 3 and 1 x 5 pixel grids (3, 9 and 15 bytes: the last dword is partial and written by bytes), and a grid of 2 x 12
    panels of 64x48 (79 blocks of 1024 pixels)."""
    viz = _viz()
    for W in (1, 3, 5):
        t = VC.fill((1, 3, 1, W), W, False)
        got = viz.grid_u8([viz.Panel(t.cuda(), viz.UNIT)])
        assert tuple(got.shape) == (1, 1, W, 3) and torch.equal(got.cpu(), VC.ref_grids([("unit", t)], 1))
    specs = VC.kind_cycle(12, 2, 64, 48, seed=9)
    got = viz.grid_u8([_panel(viz, h, t) for h, t in specs])
    assert got.numel() > 3 * 1024 * 70 and torch.equal(got.cpu(), VC.ref_grids(specs, 2))


def test_channels_last_view_that_ends_its_allocation_is_not_read_past_its_end():
    """A dense channels-last view with 12 / 4 channels sliced to 9..11 real ones has channel stride 1, an aligned pointer and
    strides that are multiples of 4: the kernel would read float4 groups.  Where the group of the last pixel would leave the
    storage, the panel is shown from a copy instead; the bytes are the restatement's either way."""
    viz = _viz()
    N, H, W = 2, 5, 7
    seg = VC.seg_scores(N, 9, H, W, 31)
    nhwc = seg.permute(0, 2, 3, 1).contiguous().cuda()                              # [N,H,W,9]: sx = 9, scalar reads
    p = viz.Panel(nhwc.permute(0, 3, 1, 2), viz.SEGMAP)
    assert p.sc == 1 and p.sx == 9 and p.ptr == nhwc.data_ptr()
    buf = torch.zeros(N * H * W * 12 - 3, device="cuda")                            # the last pixel holds 9 channels and ends the storage
    view = buf.as_strided((N, 9, H, W), (H * W * 12, 1, W * 12, 12))
    view.copy_(seg.cuda())
    q = viz.Panel(view, viz.SEGMAP)
    assert q.sc != 1 and q.ptr != buf.data_ptr()                                   # shown from an NCHW copy
    whole = torch.zeros(N * H * W * 12, device="cuda")
    view2 = whole.as_strided((N, 9, H, W), (H * W * 12, 1, W * 12, 12))
    view2.copy_(seg.cuda())
    r = viz.Panel(view2, viz.SEGMAP)
    assert r.sc == 1 and r.ptr == whole.data_ptr()                                 # readable: no copy
    want = VC.ref_grids([("seg", seg)] * 3, N)
    assert torch.equal(viz.grid_u8([p, q, r]).cpu(), want)


def test_panel_and_grid_argument_checks():
    viz = _viz()
    from hr_viton_amd.ops import HrvError
    a = torch.zeros(2, 3, 8, 8, device="cuda")
    with pytest.raises(ValueError):
        viz.grid_u8([])
    with pytest.raises(ValueError):
        viz.grid_u8([viz.Panel(a, viz.SIGNED)] * 17)
    with pytest.raises(ValueError):
        viz.grid_u8([viz.Panel(a, viz.SIGNED), viz.Panel(torch.zeros(2, 3, 8, 9, device="cuda"), viz.SIGNED)])
    with pytest.raises(ValueError):
        viz.grid_u8([viz.Panel(a, viz.SIGNED), viz.Panel(torch.zeros(3, 3, 8, 8, device="cuda"), viz.SIGNED)])
    with pytest.raises(ValueError):
        viz.Panel(torch.zeros(2, 2, 8, 8, device="cuda"), viz.UNIT)
    with pytest.raises(ValueError):
        viz.Panel(torch.zeros(2, 21, 8, 8, device="cuda"), viz.SEGMAP)
    with pytest.raises(HrvError):
        viz.Panel(a.double(), viz.SIGNED)
    with pytest.raises(HrvError):
        viz.Panel(a.cpu(), viz.SIGNED)


# ----------------------------------------------------------------------------------------- the host module
def test_visualize_segmap_equals_the_pil_chain():
    viz = _viz()
    x = VC.seg_scores(3, 13, 33, 25, 11)
    for b in range(3):
        got = viz.visualize_segmap(x.cuda(), batch=b)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, 33, 25)
        assert torch.equal(got.cpu(), VC.ref_visualize_segmap(x, batch=b))
    act = _act(x, 16, pad_value=1e9)
    assert torch.equal(viz.visualize_segmap(act, batch=2).cpu(), VC.ref_visualize_segmap(x, batch=2))


@pytest.mark.parametrize("C", [3, 1])
def test_save_images_files_are_byte_identical(tmp_path, C):
    viz = _viz()
    import test_generator as tg
    t = VC.fill((3, C, 64, 48), 21 + C, True).cuda()
    names = ["a_b.png", "c_d.png", "e_f.png"]
    old, new, thr = tmp_path / "old", tmp_path / "new", tmp_path / "thr"
    for d in (old, new, thr):
        d.mkdir()
    tg.save_images(t, names, str(old))                          # test_generator.py's host expression (utils.py:93-109)
    viz.save_images(t, names, str(new))
    with viz.ImageWriter(2) as w:
        viz.save_images(t, names, str(thr), w)
    for n in names:
        want = (old / n).read_bytes()
        assert (new / n).read_bytes() == want and (thr / n).read_bytes() == want
        assert Image.open(new / n).format == "JPEG"
    # the quantised tensor itself
    q = viz.quantize_images(t).cpu()
    for i in range(3):
        a = VC.save_images_array(t[i].cpu())
        assert np.array_equal(q[i].numpy()[..., 0] if C == 1 else q[i].numpy(), a)


# ----------------------------------------------------------------------------------------- the reference's three grids
def _opt(H=256, W=192):
    return Namespace(cuda=True, warp_feature="T1", out_layer="relu", norm_G="spectralaliasinstance", gen_semantic_nc=7, ngf=8,
                     num_upsampling_layers="more", fine_height=H, fine_width=W, occlusion=False, GT=False,
                     clothmask_composition="warp_grad", datasetting="unpaired")


@pytest.fixture(scope="module")
def tryon_case():
    """tryon_step at 256x192, ngf 8, tocg_ngf 16, batch 2: computed once, read by the three grid tests, left unchanged."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.network_generator import SPADEGenerator
    from hr_viton_amd.networks import ConditionGenerator
    from hr_viton_amd.pipeline import make_generator_inputs, tryon_step
    import test_generator as tg
    viz = _viz()
    opt = _opt()
    torch.manual_seed(0)
    tocg = ConditionGenerator(opt, 4, 16, 13, ngf=16, norm_layer=nn.BatchNorm2d)
    with torch.no_grad():
        for fc in tocg.flow_conv:
            fc.weight.mul_(4.0)
    gen = SPADEGenerator(opt, 9)
    gen.init_weights("xavier", 0.02)
    tocg.cuda().eval()
    gen.cuda().eval()
    raw = next(tg.synthetic_batches(Namespace(fine_height=256, fine_width=192, batch_size=2, datasetting="unpaired"), 2, seed=3))
    dev = {"cloth": raw["cloth"]["unpaired"].cuda(), "cloth_mask": raw["cloth_mask"]["unpaired"].cuda(),
           "parse_agnostic": raw["parse_agnostic"].cuda(), "densepose": raw["densepose"].cuda(), "agnostic": raw["agnostic"].cuda(),
           "pose": raw["pose"].cuda(), "image": raw["image"].cuda(), "parse": raw["parse"].cuda()}
    res = tryon_step(opt, tocg, gen, dev)
    g = torch.Generator().manual_seed(5)
    dev["pcm"] = (torch.rand(2, 1, 256, 192, generator=g) > 0.5).float().cuda()
    dev["parse_cloth"] = (torch.rand(2, 3, 256, 192, generator=g) * 2 - 1).cuda()
    fields_c = viz.condition_fields(opt, tocg, dev)
    aux = {}
    with torch.no_grad():
        x, parse7 = make_generator_inputs(opt, tocg, dev, aux=aux)
    return opt, dev, res, fields_c, aux, x


def _cpu(t):
    from hr_viton_amd import ops
    from hr_viton_amd.ops import Act
    return ops.to_nchw(t).cpu() if isinstance(t, Act) else t.detach().cpu()


def test_tryon_grid_equals_the_restatement(tryon_case):
    viz = _viz()
    opt, dev, res, _, _, _ = tryon_case
    from hr_viton_amd.ops import Act
    assert isinstance(res["fake_parse_gauss"], Act) and res["fake_parse_gauss"].cstride == 16 and res["fake_parse_gauss"].C == 13
    cm = (dev["cloth_mask"].cpu() > 0.5).float()
    specs = [("signed_a", _cpu(dev["cloth"])), ("mask", cm), ("seg", _cpu(dev["parse_agnostic"])), ("signed_b", _cpu(dev["densepose"])),
             ("signed_a", _cpu(res["warped_cloth"])), ("mask", _cpu(res["warped_clothmask"])), ("seg", _cpu(res["fake_parse_gauss"])),
             ("signed_a", _cpu(dev["pose"])),
             ("signed_a", _cpu(res["warped_cloth"])), ("signed_a", _cpu(dev["agnostic"])), ("signed_a", _cpu(dev["image"])),
             ("signed_a", _cpu(res["output"]))]
    got = viz.tryon_grid(dev, res)
    assert tuple(got.shape) == (2, 3 * 258 + 2, 4 * 194 + 2, 3)
    assert torch.equal(got.cpu(), VC.ref_grids(specs, 2, 4, 2, VC.ROUND))
    assert torch.equal(viz.tryon_grid(dev, res, quant=viz.TRUNC).cpu(), VC.ref_grids(specs, 2, 4, 2, VC.TRUNC))
    assert len({tuple(p[1].shape[2:]) for p in specs}) == 1 and float(_cpu(res["output"]).abs().max()) > 0


def test_condition_grid_equals_the_restatement(tryon_case):
    viz = _viz()
    opt, dev, _, f, _, _ = tryon_case
    cm = (dev["cloth_mask"].cpu() > 0.5).float()
    specs = [("signed_a", _cpu(dev["cloth"])), ("mask", cm), ("seg", _cpu(dev["parse_agnostic"])), ("signed_b", _cpu(dev["densepose"])),
             ("signed_a", _cpu(dev["parse_cloth"])), ("mask", _cpu(dev["pcm"])), ("signed_a", _cpu(f["warped_cloth"])),
             ("mask", _cpu(f["warped_cm_onehot"])),
             ("seg", _cpu(dev["parse"])), ("seg", _cpu(f["fake_segmap"])), ("signed_a", _cpu(dev["image"])), ("mask", _cpu(f["misalign"]))]
    assert set(torch.unique(_cpu(f["misalign"])).tolist()) <= {0.0, 1.0} and tuple(f["misalign"].shape) == (2, 1, 256, 192)
    assert torch.equal(viz.condition_grid(dev, f).cpu(), VC.ref_grids(specs, 2, 4, 2, VC.ROUND))
    # train_images: sample 0 alone; a long misalign (test_condition.py's) gives the same bytes
    f2 = dict(f, misalign=f["misalign"].long())
    assert torch.equal(viz.condition_grid(dev, f2, quant=viz.TRUNC, count=1).cpu(), VC.ref_grids(specs, 1, 4, 2, VC.TRUNC))


def test_generator_train_grid_equals_the_restatement(tryon_case):
    viz = _viz()
    opt, dev, res, _, aux, x = tryon_case
    assert aux["warped_cloth"].data_ptr() == x[:, 6:9].data_ptr() and not aux["warped_cloth"].is_contiguous()   # a view, no copy
    out = res["output"]
    cm = (dev["cloth_mask"].cpu() > 0.5).float()
    specs = [("signed_a", _cpu(dev["cloth"])), ("mask", cm), ("signed_b", _cpu(dev["densepose"])), ("seg", _cpu(dev["parse_agnostic"])),
             ("signed_a", x[:, 6:9].cpu()), ("signed_a", _cpu(dev["agnostic"])), ("signed_a", _cpu(dev["densepose"])),
             ("seg", _cpu(aux["fake_parse_gauss"])),
             ("signed_a", _cpu(out)), ("signed_a", _cpu(dev["image"]))]
    got = viz.generator_train_grid(dev, aux, out)
    assert tuple(got.shape) == (2, 3 * 258 + 2, 4 * 194 + 2, 3)
    assert torch.equal(got.cpu(), VC.ref_grids(specs, 2, 4, 2, VC.ROUND))
    assert int(got[:, 2 * 258 + 2:, 2 * 194 + 2:].max()) == 0                        # the two empty cells of the last row


def test_generator_fields_leave_state_and_random_streams_alone(tryon_case):
    """The recording block's eval pass: spectral-norm u / v, every parameter and buffer, the modes and the CPU and device random
    streams are what they were; the pass itself is repeatable."""
    viz = _viz()
    from hr_viton_amd.network_generator import SPADEGenerator
    opt, dev, _, _, _, _ = tryon_case
    from hr_viton_amd.networks import ConditionGenerator
    torch.manual_seed(1)
    tocg = ConditionGenerator(opt, 4, 16, 13, ngf=16, norm_layer=nn.BatchNorm2d).cuda().eval()
    gen = SPADEGenerator(opt, 9)
    gen.init_weights("xavier", 0.02)
    with torch.no_grad():
        for n_, p in gen.named_parameters():
            if n_.endswith("noise_scale"):
                p.normal_(0, 0.1)
    gen.cuda().train()
    before = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    assert any(k.endswith("weight_u") for k in before)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    f1, o1 = viz.generator_fields(opt, tocg, gen, dev)
    f2, o2 = viz.generator_fields(opt, tocg, gen, dev)
    assert gen.training is True and tocg.training is False
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), dev_state)
    for k, v in before.items():
        assert torch.equal(gen.state_dict()[k], v), k
    assert torch.equal(o1, o2) and torch.isfinite(o1).all()


# ----------------------------------------------------------------------------------------- scripts
def _check_grid_png(path, H, W):
    im = np.asarray(Image.open(path))
    assert im.shape == (3 * (H + 2) + 2, 4 * (W + 2) + 2, 3) and im.dtype == np.uint8
    for r in range(4):
        assert (im[r * (H + 2):r * (H + 2) + 2] == 0).all()                           # border rows
    for c in range(5):
        assert (im[:, c * (W + 2):c * (W + 2) + 2] == 0).all()                        # border columns
    assert im.max() > 0
    return im


def test_write_grids_generator(tmp_path):
    import test_generator as tg
    import write_grids as wg
    out, grid, out2, grid2 = tmp_path / "out", tmp_path / "grid", tmp_path / "out2", tmp_path / "grid2"
    argv = ["--synthetic", "3", "-b", "2", "--fine_height", "256", "--fine_width", "192", "--num_upsampling_layers", "more",
            "--random_init_tocg", "--gen_checkpoint", "", "--tocg_ngf", "16", "--ngf", "8", "--output_dir"]
    torch.manual_seed(0)
    assert wg.main(["generator", "--grid_dir", str(grid), "--image_workers", "2", "--with_outputs"] + argv + [str(out)]) == 3
    files = sorted(os.listdir(grid))
    assert files == sorted(os.listdir(out)) and len(files) == 3 and all(f.endswith(".png") for f in files)
    for f in files:
        assert Image.open(grid / f).format == "PNG" and Image.open(out / f).format == "JPEG"
        _check_grid_png(grid / f, 256, 192)
    # test_generator.py itself from the same seed: the same names and the same JPEG bytes, and no grid
    torch.manual_seed(0)
    tg.main(argv + [str(out2)])
    assert sorted(os.listdir(out2)) == files
    for f in files:
        assert (out2 / f).read_bytes() == (out / f).read_bytes(), f
    # without --with_outputs: grids alone, the same pixels
    torch.manual_seed(0)
    wg.main(["generator", "--grid_dir", str(grid2)] + argv + [str(tmp_path / "never")])
    assert sorted(os.listdir(tmp_path)) == ["grid", "grid2", "out", "out2"]
    for f in files:
        assert np.array_equal(np.asarray(Image.open(grid2 / f)), np.asarray(Image.open(grid / f)))


def test_write_grids_condition(tmp_path):
    import write_grids as wg
    grid = tmp_path / "grid"
    n = wg.main(["condition", "--grid_dir", str(grid), "--synthetic", "-b", "2", "--num_batches", "2", "--ngf", "8",
                 "--output_dir", str(tmp_path / "o")])
    files = sorted(os.listdir(grid))
    assert n == 4 and files == ["synthetic_%05d.png" % k for k in range(4)]
    ims = [_check_grid_png(grid / f, 256, 192) for f in files]
    assert not np.array_equal(ims[0], ims[1])
    assert sorted(os.listdir(tmp_path)) == ["grid"]                                   # no rejection file, no output tree


GEN_ARGV = ["--synthetic", "-b", "2", "--fine_height", "256", "--fine_width", "192", "--num_upsampling_layers", "more", "--ngf", "8",
            "--ndf", "8", "--tocg_ngf", "8", "--max_steps", "2", "--num_test_visualize", "2"]
GEN_TAGS = ["Loss/gen", "Loss/gen/adv", "Loss/gen/feat", "Loss/gen/vgg", "Loss/dis", "Loss/dis/adv_fake", "Loss/dis/adv_real"]


def _run_tg(tmp_path, name, extra):
    import train_generator as tg
    torch.manual_seed(0)
    tg.main(["--name", name, "--checkpoint_dir", str(tmp_path / "ck"), "--tensorboard_dir", str(tmp_path / "tb")] + GEN_ARGV + extra)
    return torch.load(str(tmp_path / "ck" / name / "gen_model_final.pth"), map_location="cpu")


def test_train_generator_board(tmp_path):
    from hr_viton_amd import validate as V
    sd_board = _run_tg(tmp_path, "b", ["--board", "--tensorboard_count", "1"])
    recs = V.read_scalars(str(tmp_path / "tb" / "b"))
    for step in (1, 2):
        assert [r["tag"] for r in recs if r["step"] == step] == GEN_TAGS
    assert len(recs) == 2 * len(GEN_TAGS) and all(np.isfinite(r["value"]) for r in recs)
    img = tmp_path / "tb" / "b" / "images"
    assert sorted(os.listdir(img)) == ["test_images_0", "test_images_1", "train_images"]
    for d in ("train_images", "test_images_0", "test_images_1"):
        assert sorted(os.listdir(img / d)) == ["00000001.png", "00000002.png"]
        _check_grid_png(img / d / "00000001.png", 256, 192)
    # the same run without --board: no record, no image, and bitwise the same generator (the eval pass moved neither the
    # spectral-norm vectors nor the random streams the training draws its SPADE noise from)
    sd_plain = _run_tg(tmp_path, "p", ["--tensorboard_count", "1"])
    assert not (tmp_path / "tb" / "p").exists()
    assert list(sd_plain) == list(sd_board) and any(k.endswith("weight_u") for k in sd_plain)
    for k in sd_plain:
        assert torch.equal(sd_plain[k], sd_board[k]), k
    # a switched-off loss is skipped
    _run_tg(tmp_path, "n", ["--board", "--tensorboard_count", "2", "--no_vgg_loss", "--no_ganFeat_loss", "--num_test_visualize", "0"])
    recs = V.read_scalars(str(tmp_path / "tb" / "n"))
    assert [r["tag"] for r in recs] == [t for t in GEN_TAGS if t not in ("Loss/gen/feat", "Loss/gen/vgg")]
    assert all(r["step"] == 2 for r in recs) and sorted(os.listdir(tmp_path / "tb" / "n" / "images")) == ["train_images"]


COND_ARGV = ["--synthetic", "-b", "2", "--ngf", "8", "--max_steps", "2", "--num_test_visualize", "2"]
COND_TAGS = ["Loss/G", "Loss/G/l1_cloth", "Loss/G/vgg", "Loss/G/tv", "Loss/G/CE", "Loss/G/GAN", "Loss/D", "Loss/D/pred_real",
             "Loss/D/pred_fake"]


def _run_tc(tmp_path, name, extra):
    import train_condition as tc
    torch.manual_seed(0)
    tc.main(["--name", name, "--checkpoint_dir", str(tmp_path / "ck"), "--tensorboard_dir", str(tmp_path / "tb")] + COND_ARGV + extra)
    return torch.load(str(tmp_path / "ck" / name / "tocg_final.pth"), map_location="cpu")


def test_train_condition_board(tmp_path):
    from hr_viton_amd import validate as V
    sd = _run_tc(tmp_path, "b", ["--board", "--tensorboard_count", "1"])
    recs = V.read_scalars(str(tmp_path / "tb" / "b"))
    for step in (1, 2):
        assert [r["tag"] for r in recs if r["step"] == step] == COND_TAGS
    assert len(recs) == 2 * len(COND_TAGS) and all(np.isfinite(r["value"]) for r in recs)
    img = tmp_path / "tb" / "b" / "images"
    assert sorted(os.listdir(img)) == ["test_images_0", "test_images_1", "train_images"]
    for d in ("train_images", "test_images_0", "test_images_1"):
        assert sorted(os.listdir(img / d)) == ["00000001.png", "00000002.png"]
        _check_grid_png(img / d / "00000002.png", 256, 192)
    assert int(sd["out_layer.block.1.num_batches_tracked"]) == 2                     # two training steps; the eval passes added none
    # --no_test_visualize, --no_GAN_loss, --no_vgg_loss
    _run_tc(tmp_path, "n", ["--board", "--tensorboard_count", "2", "--no_test_visualize", "--no_GAN_loss", "--no_vgg_loss"])
    recs = V.read_scalars(str(tmp_path / "tb" / "n"))
    assert [r["tag"] for r in recs] == ["Loss/G", "Loss/G/l1_cloth", "Loss/G/tv", "Loss/G/CE"] and all(r["step"] == 2 for r in recs)
    assert sorted(os.listdir(tmp_path / "tb" / "n" / "images")) == ["train_images"]


def test_condition_recording_leaves_networks_and_random_streams_alone(tmp_path):
    """What ``train_generator.py --board`` is held to by comparing two runs is held here on the recording block itself, because two
    runs of ``train_condition.py`` from one seed are not bitwise equal with or without ``--board``: the flow warp's backward scatters
    with float atomics (cond_train.py).  Measured on an MI355X, 2 steps, ngf 8, batch 2: plain against plain 177 of tocg's 262
    tensors differ (max 2.4e-5) and 18 of D's 20 (3.4e-4); plain against ``--board`` 174 of 262 (2.2e-4) and 18 of 20 (3.4e-4).
    So: after a real training step, ``record`` (loss scalars, ``train_images``, the eval-mode pass and ``test_images/{i}``) leaves every
    parameter and buffer of tocg and D -- BatchNorm's running statistics and ``num_batches_tracked`` among them -- the optimizers'
    state, the modes and the CPU and device random streams bitwise as they were."""
    import train_condition as tc
    from hr_viton_amd.losses import L1Loss
    from hr_viton_amd.networks import ConditionGenerator, GANLoss, define_D
    from hr_viton_amd.optim import Adam
    from hr_viton_amd.pipeline import condition_train_step
    opt = tc.get_opt(["--name", "r", "--synthetic", "-b", "2", "--ngf", "8", "--num_test_visualize", "2", "--board", "--no_vgg_loss",
                      "--spectral", "--occlusion", "--tensorboard_dir", str(tmp_path / "tb")])
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    tocg = ConditionGenerator(opt, input1_nc=4, input2_nc=16, output_nc=13, ngf=opt.ngf, norm_layer=nn.BatchNorm2d).to(dev).train()
    D = define_D(input_nc=4 + 16 + 13, Ddownx2=opt.Ddownx2, Ddropout=opt.Ddropout, n_layers_D=3, spectral=opt.spectral,
                 num_D=opt.num_D).to(dev).train()
    opt_g, opt_d = Adam(tocg.parameters(), lr=opt.G_lr, betas=(0.5, 0.999)), Adam(D.parameters(), lr=opt.D_lr, betas=(0.5, 0.999))
    batch = tc.synthetic_batch(opt, 2, 11, dev)
    batch["image"] = tc.synthetic_image(opt, 2, 11, dev)
    aux = {}
    losses = condition_train_step(opt, tocg, D, L1Loss(), None, GANLoss(use_lsgan=True), opt_g, opt_d, batch, aux=aux)
    assert set(aux) == {"cm_paired", "fake_segmap", "warped_cloth", "warped_cm_onehot", "misalign"}
    assert not any(v.requires_grad for v in aux.values())

    def snapshot():
        st = {"tocg." + k: v.detach().clone() for k, v in tocg.state_dict().items()}
        st.update({"D." + k: v.detach().clone() for k, v in D.state_dict().items()})
        for name, o in (("opt_g", opt_g), ("opt_d", opt_d)):
            for gi, grp in enumerate(o.state_dict()["state"].values()):
                for k, v in grp.items():
                    if torch.is_tensor(v):
                        st[f"{name}.{gi}.{k}"] = v.detach().clone()
        return st

    before = snapshot()
    assert any(k.endswith("running_var") for k in before) and any(k.startswith("opt_g.") for k in before)
    assert int(before["tocg.out_layer.block.1.num_batches_tracked"]) == 1
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    v = tc._Validation(opt, dev)
    v.record(tocg, 0, losses, batch, aux)
    v.record(tocg, 1, losses, batch, aux)
    v.board.close()
    assert tocg.training is True and D.training is True
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    after = snapshot()
    assert list(after) == list(before)
    for k, t in before.items():
        assert torch.equal(after[k], t), k
    img = tmp_path / "tb" / "r" / "images"
    assert sorted(os.listdir(img)) == ["test_images_0", "test_images_1", "train_images"]
    a, b = (np.asarray(Image.open(img / "test_images_0" / f)) for f in ("00000001.png", "00000002.png"))
    assert np.array_equal(a, b)                                  # the same items through unchanged networks: the same picture
    _check_grid_png(img / "train_images" / "00000001.png", 256, 192)


def test_without_the_flags_no_image_and_no_loss_record(tmp_path):
    from hr_viton_amd import validate as V
    _run_tc(tmp_path, "c", ["--tensorboard_count", "1", "--val_count", "2", "--val_items", "2", "--no_vgg_loss"])
    recs = V.read_scalars(str(tmp_path / "tb" / "c"))
    assert [r["tag"] for r in recs] == ["val/iou"] and not (tmp_path / "tb" / "c" / "images").exists()
    _run_tg(tmp_path, "g", ["--tensorboard_count", "1", "--no_vgg_loss"])
    assert not (tmp_path / "tb" / "g").exists()
