"""The class-conditional UNet and classifier-free guidance, everything that needs no GPU: the restatement's anchor, the
parameter table, the refusals of the Python mirror, the sampler's bookkeeping, the dropout draw, the labelled dataset."""
import numpy as np
import pytest
import torch

import cond_ref

N = 5


@pytest.fixture(scope="module")
def cond_sd():
    from synt_isic_amd.weights import synthetic_unet_state_dict
    return synthetic_unet_state_dict(num_class_embeds=N)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_restatement_with_a_zero_table_is_the_oracle(synthetic_sd, cond_sd):
    from oracle import unet as ounet
    sd = dict(cond_sd)
    sd[cond_ref.TABLE] = torch.zeros_like(sd[cond_ref.TABLE])
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 16, 16, generator=g)
    t = torch.tensor([37, 912])
    with torch.no_grad():
        want = ounet.unet_forward(synthetic_sd, x, t)
        got = cond_ref.unet_forward(sd, x, t, [0, 4])
        live = cond_ref.unet_forward(cond_sd, x, t, [0, 4])
        same_row = cond_ref.unet_forward(cond_sd, x, t, [4, 4])
    assert torch.equal(got, want)
    assert not torch.equal(live, want)                                  # the table reaches the output ...
    assert torch.equal(live[1], same_row[1]) and not torch.equal(live[0], same_row[0])     # ... through the sample's own row


def test_guidance_combine_restatement():
    c = np.array([1.0, -2.5, 3.0e-8, 7.0], dtype=np.float32)
    u = np.array([0.5, 4.0, -1.0, 7.0], dtype=np.float32)
    assert np.array_equal(cond_ref.guide(c, u, 0.0), u + np.float32(0.0) * (c - u))
    assert cond_ref.guide(c, u, 3.0).dtype == np.float32
    assert np.array_equal(cond_ref.guide(c, u, 3.0), np.array([2.0, -15.5, np.float32(-1.0) + np.float32(3.0) * (np.float32(3.0e-8) - np.float32(-1.0)), 7.0], dtype=np.float32))
    # w = 1 is NOT the identity on eps_c in floating point: u + (c - u) rounds twice
    big, small = np.float32(1.0e8), np.float32(1.0)
    assert cond_ref.guide(np.array([small]), np.array([big]), 1.0)[0] == np.float32(big + (small - big))


# ---- the parameter table -----------------------------------------------------------------------------------------------
def test_param_spec_gains_the_table_at_its_place():
    from synt_isic_amd.arch import UNetConfig, unet_param_spec
    plain = unet_param_spec()
    assert len(plain) == 330 and cond_ref.TABLE not in plain and UNetConfig().num_class_embeds is None
    spec = unet_param_spec(UNetConfig(num_class_embeds=N))
    names = list(spec)
    assert len(spec) == 331
    at = names.index(cond_ref.TABLE)
    assert names[at - 1] == "time_embedding.linear_2.bias" and names[at + 1] == "down_blocks.0.resnets.0.norm1.weight" and at == 6
    assert spec[cond_ref.TABLE] == (N, 256)
    assert [(k, v) for k, v in spec.items() if k != cond_ref.TABLE] == list(plain.items())
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            UNetConfig(num_class_embeds=bad).validate()


def test_synthetic_weights_keep_the_other_330_tensors(synthetic_sd, cond_sd):
    from synt_isic_amd.arch import UNetConfig, unet_param_spec
    from synt_isic_amd.weights import synthetic_unet_state_dict
    assert list(cond_sd) == list(unet_param_spec(UNetConfig(num_class_embeds=N)))
    assert all(torch.equal(cond_sd[k], v) for k, v in synthetic_sd.items())
    table = cond_sd[cond_ref.TABLE]
    assert table.shape == (N, 256) and table.dtype == torch.float32
    assert abs(float(table.mean())) < 0.15 and 0.8 < float(table.std()) < 1.2           # N(0, 1), nn.Embedding's default
    assert torch.equal(synthetic_unet_state_dict(num_class_embeds=N)[cond_ref.TABLE], table)        # seeded
    more = synthetic_unet_state_dict(num_class_embeds=N + 1)
    assert more[cond_ref.TABLE].shape == (N + 1, 256)
    assert not torch.equal(synthetic_unet_state_dict(seed=99, num_class_embeds=N)[cond_ref.TABLE], table)
    assert list(synthetic_unet_state_dict(cfg=UNetConfig(num_class_embeds=N))) == list(cond_sd)


# ---- the mirror's refusals ---------------------------------------------------------------------------------------------
def test_model_constructor_and_the_two_value_errors(synthetic_sd, cond_sd):
    from synt_isic_amd.unet import HipUNet2DModel
    with pytest.raises(NotImplementedError):
        HipUNet2DModel(class_embed_type="timestep")
    with pytest.raises(NotImplementedError):
        HipUNet2DModel(class_embed_type="identity", num_class_embeds=N)
    with pytest.raises(ValueError):
        HipUNet2DModel(num_class_embeds=0)
    m = HipUNet2DModel(num_class_embeds=N)
    assert m.config.num_class_embeds == N and len(m._spec) == 331
    m.load_state_dict(cond_sd)
    assert sum(p.numel() for p in m.parameters()) == 25_304_963 + N * 256
    with pytest.raises(RuntimeError, match="missing keys"):
        m.load_state_dict(synthetic_sd)                                 # strict: the table is required
    x = torch.zeros(3, 3, 32, 32)
    with pytest.raises(ValueError, match="class_labels should be provided"):
        m(x, 5)
    plain = HipUNet2DModel()
    plain.load_state_dict(synthetic_sd)
    with pytest.raises(RuntimeError, match="unexpected keys"):
        plain.load_state_dict(cond_sd)
    with pytest.raises(ValueError, match="class_embedding needs to be initialized"):
        plain(x, 5, class_labels=torch.tensor([0, 1, 2]))
    # label checks come before anything touches a device
    for bad in ([0, 1, N], [-1, 0, 0], [0, 1], torch.tensor([0.0, 1.0, 2.0])):
        with pytest.raises(ValueError):
            m(x, 5, class_labels=bad)
    # well-formed labels get as far as the device check
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(x, 5, class_labels=[0, 4, 2])
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(x, 5, class_labels=torch.tensor(3))                           # one label for the whole batch


# ---- the sampler -------------------------------------------------------------------------------------------------------
def test_guidance_scale_validation():
    from synt_isic_amd.sampler import Guidance, check_guidance_scale
    assert check_guidance_scale(3) == 3.0 and check_guidance_scale(-0.5) == -0.5 and check_guidance_scale(0) == 0.0
    for bad in (float("nan"), float("inf"), None, "3", True):
        with pytest.raises(ValueError):
            check_guidance_scale(bad)
    g = Guidance([0, 1], 5, 3)
    assert g.labels == (0, 1) and g.scale == 3.0 and g.null_label == 5
    with pytest.raises(ValueError):
        Guidance([0], 5, float("nan"))


def test_add_conditional_model_bookkeeping(synthetic_sd, cond_sd):
    from synt_isic_amd.sampler import Sampler, image_seed
    s = Sampler("cpu")
    names = ["MEL", "NV", "BCC", "AKIEC"]
    m = s.add_conditional_model(names, cond_sd)
    assert m.config.num_class_embeds == N == len(names) + 1
    assert all(s.models[n] is m for n in names) and s.class_labels == {"MEL": 0, "NV": 1, "BCC": 2, "AKIEC": 3}
    s.add_model("DF", synthetic_sd)
    model, per_image, g = s._resolve_classes(["MEL", "NV", "MEL"], 3, 3.0)
    assert model is m and per_image == ["MEL", "NV", "MEL"] and g.labels == (0, 1, 0) and g.null_label == 4 and g.scale == 3.0
    _, _, g = s._resolve_classes("BCC", 2, 1.0)
    assert g.labels == (2, 2) and g.scale == 1.0
    _, _, g = s._resolve_classes(["MEL", "NV"], 2, 0)                   # scale 0: null labels at scale 1, one pass
    assert g.labels == (4, 4) and g.scale == 1.0
    assert s._resolve_classes("DF", 2, 1.0)[2] is None
    with pytest.raises(ValueError, match="one entry per seed"):
        s.generate_seeds(["MEL", "NV"], [1, 2, 3], 4)
    with pytest.raises(ValueError, match="needs a class-conditional model"):
        s.generate_seeds("DF", [1], 4, guidance_scale=3.0)
    with pytest.raises(ValueError, match="one conditional model"):
        s.generate_seeds(["MEL", "DF"], [1, 2], 4)
    with pytest.raises(KeyError):
        s.generate_seeds(["MEL", "VASC"], [1, 2], 4)
    with pytest.raises(ValueError, match="finite"):
        s.generate_seeds("MEL", [1], 4, guidance_scale=float("nan"))
    with pytest.raises(ValueError, match="one entry per image"):
        s.generate(1, ["MEL", "NV"], 4, count=3)
    # registration refusals
    with pytest.raises(ValueError, match="already registered"):
        s.add_conditional_model(["NV", "VASC"], cond_sd)
    for bad in ([], "MEL", ["A", "A"]):
        with pytest.raises(ValueError):
            Sampler("cpu").add_conditional_model(bad, cond_sd)
    with pytest.raises(ValueError, match="embedding rows"):
        Sampler("cpu").add_conditional_model(["A", "B"], cond_sd, num_class_embeds=N)
    with pytest.raises(RuntimeError, match="size mismatch"):
        Sampler("cpu").add_conditional_model(["A", "B"], cond_sd)     # a 5-row table for a 3-row model
    # the per-image seed derives from the image's own class name
    assert image_seed(7, "MEL", 0) != image_seed(7, "NV", 0)


def test_run_sampling_loop_checks_guidance(synthetic_sd, cond_sd):
    from synt_isic_amd.sampler import Guidance, _check_guidance
    from synt_isic_amd.unet import HipUNet2DModel
    m, plain = HipUNet2DModel(num_class_embeds=N), HipUNet2DModel()
    _check_guidance(plain, None, 3)
    _check_guidance(m, Guidance([0, 4, 2], 4, 3.0), 3)
    with pytest.raises(ValueError, match="needs? a class-conditional model"):
        _check_guidance(plain, Guidance([0], 0, 1.0), 1)
    with pytest.raises(ValueError, match="samples under labels"):
        _check_guidance(m, None, 3)
    with pytest.raises(ValueError, match="for a batch of 3"):
        _check_guidance(m, Guidance([0, 1], 4, 1.0), 3)
    with pytest.raises(ValueError, match="outside"):
        _check_guidance(m, Guidance([0, 1, N], 4, 1.0), 3)
    with pytest.raises(ValueError, match="outside"):
        _check_guidance(m, Guidance([0, 1, 2], N, 3.0), 3)


# ---- label dropout -----------------------------------------------------------------------------------------------------
def test_dropout_draw_follows_noise_and_timesteps():
    from synt_isic_amd.train import drop_labels
    shape, p, null = (6, 3, 8, 8), 0.4, N - 1
    labels = torch.tensor([0, 1, 2, 3, 0, 1])
    g = torch.Generator().manual_seed(11)
    noise, timesteps, drop = cond_ref.dropout_draw(shape, p, g)
    after = torch.rand(1, generator=g)
    # the loop's own order: randn, randint, then drop_labels' rand
    h = torch.Generator().manual_seed(11)
    assert torch.equal(torch.randn(shape, generator=h), noise)
    assert torch.equal(torch.randint(0, 1000, (shape[0],), generator=h).long(), timesteps)
    got = drop_labels(labels, p, null, h)
    assert torch.equal(got, cond_ref.drop_labels(labels, drop, null)) and got.dtype == torch.int64
    assert torch.equal(torch.rand(1, generator=h), after)               # exactly one draw of B uniforms was consumed
    assert 0 < int(drop.sum()) < shape[0]                               # the seed exercises both branches
    # a function of the generator: the same seed gives the same mask, another seed another
    assert torch.equal(drop_labels(labels, p, null, torch.Generator().manual_seed(3)), drop_labels(labels, p, null, torch.Generator().manual_seed(3)))
    masks = {tuple(drop_labels(labels, 0.5, null, torch.Generator().manual_seed(k)).tolist()) for k in range(8)}
    assert len(masks) > 1
    # p = 0 keeps every label and still consumes the draw; p = 1 drops all
    k = torch.Generator().manual_seed(11)
    assert torch.equal(drop_labels(labels, 0.0, null, k), labels)
    assert torch.equal(torch.rand(1, generator=k), torch.rand(7, generator=torch.Generator().manual_seed(11))[6:])
    assert torch.equal(drop_labels(labels, 1.0, null, torch.Generator().manual_seed(1)), torch.full_like(labels, null))
    with pytest.raises(ValueError):
        drop_labels(labels, 1.5, null)


def test_train_conditional_refuses_the_wrong_model(synthetic_sd, cond_sd):
    from synt_isic_amd import train
    from synt_isic_amd.unet import HipUNet2DModel
    with pytest.raises(ValueError, match="class-conditional"):
        train.train_conditional(HipUNet2DModel(), [], "all")
    with pytest.raises(ValueError, match="cond_drop_prob"):
        train.train_conditional(HipUNet2DModel(num_class_embeds=N), [], "all", cond_drop_prob=-0.1)
    with pytest.raises(ValueError, match="train_conditional"):
        train.train_class(HipUNet2DModel(num_class_embeds=N), [], "NV")


# ---- the labelled dataset ----------------------------------------------------------------------------------------------
def test_device_dataset_checks_labels_before_the_device():
    from synt_isic_amd.data import DeviceDataset
    imgs = np.zeros((4, 8, 8, 3), dtype=np.uint8)
    for bad in ([0, 1, 2], np.zeros(5, dtype=np.int64), [0.0, 1.0, 2.0, 3.0], [[0, 1], [2, 3]], [0, 1, 2, -1]):
        with pytest.raises(ValueError):
            DeviceDataset(imgs, device="cpu", labels=bad)
    # well-formed labels get as far as the device check, as an unlabelled dataset does
    for labels in (None, [0, 1, 2, 3], torch.tensor([3, 3, 0, 1])):
        with pytest.raises(RuntimeError, match="MI355X"):
            DeviceDataset(imgs, device="cpu", labels=labels)
    with pytest.raises(ValueError, match="distinct"):
        DeviceDataset.from_isic_classes("nowhere", "nothing.csv", [1, 1])
    with pytest.raises(ValueError, match="non-empty"):
        DeviceDataset.from_isic_classes("nowhere", "nothing.csv", [])
