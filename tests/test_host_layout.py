"""Host-side weight-layout logic of lab4d_amd/mlp.py on CPU (no launches): the column maps that turn reference-layout
(checkpoint compatible) weights into the kernels' input order must consume every reference column exactly once -- embedding
block through the slot permutation, conditioning block through the per-frame bias, previous activations in order -- and
the slot permutation must agree with the reference's PosEmbedding channel layout (embedding.py:96-108, pinned for the
oracle by tests/golden/ops.pt).  lab4d_mlp_describe is a host function of the library (no GPU needed)."""
import torch

from lab4d_amd import mlp, synthetic
from oracle import lab4d_oracle as O


def all_weights():
    P = synthetic.add_dense_weights(synthetic.make_weights(0))
    P.update({"bg." + k: v for k, v in synthetic.make_bg_weights(0).items()})
    P.update({"d6." + k: v for k, v in synthetic.make_weights(0, motion="dense").items() if k.startswith("warp.")})  # fg_motion "dense"
    return P


CASES = [(mlp.NET_FG_BASE, ""), (mlp.NET_FG_COLOR, ""), (mlp.NET_VIS, ""), (mlp.NET_FEAT, ""), (mlp.NET_SKIN, ""),
         (mlp.NET_DENSE, "warp.post_warp.forward_map."), (mlp.NET_DENSE, "warp.post_warp.backward_map."),
         (mlp.NET_BG_BASE, "bg."), (mlp.NET_BG_COLOR, "bg."), (mlp.NET_DENSE6, "d6.warp.forward_map."), (mlp.NET_DENSE6, "d6.warp.backward_map.")]


def test_every_reference_weight_column_is_consumed_exactly_once():
    P = all_weights()
    for net, prefix in CASES:
        d = mlp.describe(net)
        bds = mlp.bindings(net, prefix)
        assert len(bds) == d.n_layers, (net, len(bds), d.n_layers)
        for layer, bd in enumerate(bds):
            W = P[bd.wname]
            L = d.layers[layer]
            assert W.shape[0] == L.mout, (bd.wname, W.shape, L.mout)
            cm = mlp.col_map(net, layer, "cpu").tolist()
            assert len(cm) == L.ke + L.kin
            used = [c for c in cm if c >= 0]
            assert len(used) == len(set(used)), bd.wname
            cond = list(range(bd.cond[0], bd.cond[0] + bd.cond[1])) if bd.cond else []
            assert not set(used) & set(cond), bd.wname
            assert sorted(used + cond) == list(range(W.shape[1])), (bd.wname, W.shape[1], len(used), len(cond))
            assert bool(L.pf_bias) == bool(bd.cond), bd.wname


def test_affine_form_skin_nets_bind_the_reference_layers_two_and_final():
    """LAB4D_NET_SKIN_A / _SKIN18_A: layers 0 / 1 are the reference's linear_2 / linear_final with identity column maps (the 64 "embedding" slots
    are the hidden features of the folded linear_1, in order); the folded layer's columns are consumed by warping.skin_affine_table."""
    for n_bones, net_old in ((25, mlp.NET_SKIN), (18, mlp.NET_SKIN18)):
        net = mlp.skin_net_for(n_bones, affine=True)
        assert net in (mlp.NET_SKIN_A, mlp.NET_SKIN18_A) and mlp.skin_net_for(n_bones) == net_old
        d, old = mlp.describe(net), mlp.describe(net_old)
        assert d.emb_kind == 2 and d.n_layers == old.n_layers - 1 and d.c_out == n_bones and d.ke == old.layers[0].mout_pad == 64
        bd, bd_old = mlp.bindings(net), mlp.bindings(net_old)
        assert [b.wname for b in bd] == [b.wname for b in bd_old[1:]]
        for layer in range(d.n_layers):
            L = d.layers[layer]
            assert (L.mout, L.relu, L.pf_bias) == (old.layers[layer + 1].mout, old.layers[layer + 1].relu, 0)
            assert mlp.col_map(net, layer, "cpu").tolist() == list(range(L.ke + L.kin))


def test_slot_permutation_matches_the_reference_embedding_layout():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(9, 3, generator=g)
    for n_freq in (6, 8, 10, 12):
        ref = O.pos_embedding(x, n_freq)  # reference channel order
        ke = (6 * n_freq + 3 + 31) // 32 * 32
        chan = mlp.posenc_slot_to_ref_channel(n_freq, ke)
        assert sorted(c for c in chan if c >= 0) == list(range(6 * n_freq + 3))
        for slot, c in enumerate(chan):
            if slot < 6 * n_freq:  # the kernel's slot contents: pairs (sin, cos) of one (frequency, axis)
                pair, t = slot >> 1, slot & 1
                f, a = pair // 3, pair % 3
                val = torch.sin(x[:, a] * 2.0 ** f) if t == 0 else torch.cos(x[:, a] * 2.0 ** f)
            elif slot < 6 * n_freq + 3:
                val = x[:, slot - 6 * n_freq]
            else:
                assert c == -1
                continue
            assert torch.allclose(ref[:, c], val, atol=1e-6), (n_freq, slot, c)


def test_first_layer_through_the_column_map_equals_the_reference_layer():
    """W[:, col_map] applied to the slot-ordered embedding + the per-frame bias == F.linear on [posenc | code] (CondMLP, base.py:139-146)."""
    P = all_weights()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(5, 3, generator=g)
    for net, prefix, n_freq, wname, code_name in [(mlp.NET_FG_BASE, "", 10, "basefield.linear_1.0", "basefield.inst_embedding.mapping.weight"),
                                                  (mlp.NET_VIS, "", 10, "vis_mlp.basefield.linear_1.0", "vis_mlp.basefield.inst_embedding.mapping.weight"),
                                                  (mlp.NET_BG_BASE, "bg.", 6, "bg.basefield.linear_1.0", "bg.basefield.inst_embedding.mapping.weight")]:
        W, b, code = P[wname + ".weight"], P[wname + ".bias"], P[code_name][:1]
        ref = torch.nn.functional.linear(torch.cat([O.pos_embedding(x, n_freq), code.expand(5, -1)], -1), W, b)
        cm = mlp.col_map(net, 0, "cpu")
        emb_ref = O.pos_embedding(x, n_freq)
        chan = mlp.posenc_slot_to_ref_channel(n_freq, len(cm))
        slots = torch.stack([emb_ref[:, c] if c >= 0 else torch.zeros(5) for c in chan], -1)  # what the kernel computes per slot
        Wk = torch.stack([W[:, c] if c >= 0 else torch.zeros(W.shape[0]) for c in cm.tolist()], -1)  # what lab4d_mlp_pack gathers
        got = slots @ Wk.t() + mlp.pf_bias_of(net, 0, W, code) + b
        assert torch.allclose(got, ref, atol=1e-5), wname


# The per-net tables as they stood before they were derived from mlp.NETS (bench.py, the tests and tools/ read them by these names).
NET_NAMES = {0: "fg_base", 1: "fg_color", 2: "vis", 3: "feat", 4: "skin", 5: "dense", 6: "bg_base", 7: "bg_color", 8: "skin18", 9: "hash_geo", 10: "hash_color", 11: "dense6",
             12: "skin_a", 13: "skin18_a"}
KERNEL_NET = {0: "FgBase", 1: "FgColor", 2: "Vis", 3: "Feat", 4: "Skin", 5: "Dense", 6: "BgBase", 7: "BgColor", 8: "Skin18", 9: "HashGeo", 10: "HashColor", 11: "Dense6", 12: "SkinA",
              13: "Skin18A"}
NET_MACS = {0: 572928 + 256, 1: 158464 + 37248, 2: 10240, 3: 77568, 4: 20736, 5: 39 * 256 + 256 * 256 + 256 * 3,
            6: 100096 + 128, 7: 43392 + 8576, 8: (54 + 160) * 64 + 64 * 64 + 64 * 18, 9: 32 * 64 + 64 * 16, 10: 19 * 64 + 64 * 64 + 64 * 3,
            11: 199 * 256 + 3 * 256 * 256 + 455 * 256 + 256 * 256 + 256 * 3,
            12: 4 * 64 + 64 * 64 + 64 * 25, 13: 4 * 64 + 64 * 64 + 64 * 18}
WS_NETS = (0, 1, 5, 11)


def test_per_net_tables_keep_their_contents():
    """NET_NAMES, KERNEL_NET, NET_MACS and WS_NETS are derived from one record per net (mlp.NETS): same keys, types and values as the literal
    tables they replace, and the NET_* constants name the same ids."""
    assert mlp.NET_NAMES == NET_NAMES and mlp.KERNEL_NET == KERNEL_NET and mlp.NET_MACS == NET_MACS
    for table in (mlp.NET_NAMES, mlp.KERNEL_NET, mlp.NET_MACS):
        assert type(table) is dict and list(table) == list(range(14))
    assert mlp.WS_NETS == WS_NETS and type(mlp.WS_NETS) is tuple
    assert all(type(v) is int for v in mlp.NET_MACS.values())
    assert {n: getattr(mlp, "NET_" + name.upper()) for n, name in NET_NAMES.items()} == {n: n for n in range(14)}


def test_bindings_of_every_net_match_the_recorded_ones(golden_dir):
    """bindings(net) for all 14 nets against tests/golden/mlp_bindings.json -- (wname, bname, emb0, cond, prev0, aux0) per layer, recorded from the
    one-branch-per-net form of bindings() before it was built from the two layer-pattern helpers -- and against the library's own description:
    one binding per layer, a conditioning block exactly where the layer takes a per-frame bias."""
    import json
    import os
    snap = json.load(open(os.path.join(golden_dir, "mlp_bindings.json")))
    assert sorted(snap) == sorted(NET_NAMES.values())
    for net, name in NET_NAMES.items():
        d, bds = mlp.describe(net), mlp.bindings(net)
        assert len(bds) == d.n_layers, name
        assert [[b.wname, b.bname, b.emb0, list(b.cond) if b.cond else None, b.prev0, b.aux0] for b in bds] == snap[name], name
        for layer, b in enumerate(bds):
            assert bool(d.layers[layer].pf_bias) == (b.cond is not None), (name, layer)
        assert [(b.wname, b.bname) for b in mlp.bindings(net, "pre.")] == [("pre." + b.wname, "pre." + b.bname) for b in bds], name


def test_mask_numel_is_one_lane_word_per_tile_and_32_features():
    for prec, tile in ((mlp.PREC_BF16, 64), (mlp.PREC_F32, 32)):
        for mout_pad in (32, 64, 256):
            for S_pad in (256, 512):
                L = mlp.LayerDesc(mout_pad=mout_pad)
                assert mlp.mask_numel(L, S_pad, prec) == (S_pad // tile) * (mout_pad // 32) * 64
