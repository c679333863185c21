"""Host-side logic that needs no GPU: constructor signatures, state_dict keys (vs the reference's, captured
in tests/golden/keys.npz), offsets, lengths, aliases, error behaviour, patch()."""
import os
import sys
import types

import pytest
import torch
import torch.nn as nn

from oracle import cpu_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_keys_match_reference(golden):
    from torecsys_amd import inputs as I, layers as L
    K = golden("keys")
    built = {
        "multi": I.MultiIndicesEmbedding(embed_size=4, field_sizes=[3, 4]),
        "single": I.SingleIndexEmbedding(embed_size=4, field_size=5),
        "fa": I.MultiIndicesFieldAwareEmbedding(embed_size=4, field_sizes=[3, 4]),
        "fm": L.FactorizationMachineLayer(),
        "ffm": L.FieldAwareFactorizationMachineLayer(num_fields=3),
        "ipn": L.InnerProductNetworkLayer(num_fields=3),
        "cross": L.CrossNetworkLayer(inputs_size=4, num_layers=2),
        "cin": L.CompressInteractionNetworkLayer(embed_size=4, num_fields=3, output_size=1, layer_sizes=[2, 2]),
    }
    for k, m in built.items():
        ref = [s for s in K("keys/" + k) if s]
        assert list(m.state_dict().keys()) == ref, k


def test_offsets_lengths_and_attrs():
    from torecsys_amd.inputs import MultiIndicesEmbedding, MultiIndicesFieldAwareEmbedding, SingleIndexEmbedding
    fs = [3, 5, 2, 7]
    m = MultiIndicesEmbedding(embed_size=8, field_sizes=fs)
    assert torch.equal(m.offsets, O.field_offsets(fs)) and m.offsets.dtype == torch.int64
    assert (m.field_size, m.embed_size, m.padding_idx, len(m)) == (17, 8, None, 8)
    assert len(MultiIndicesEmbedding(embed_size=8, field_sizes=fs, flatten=True)) == 32
    assert "offsets" not in m.state_dict()
    # offsets beyond 2**24 rows stay exact (the reference's float32 round trip does not)
    big = [20_000_001, 30_000_001, 5]
    assert MultiIndicesEmbedding.__init__.__defaults__ is not None
    assert O.field_offsets(big).tolist() == [0, 20_000_001, 50_000_002]
    assert O.field_offsets(big, through_float32=True).tolist() != [0, 20_000_001, 50_000_002]
    fa = MultiIndicesFieldAwareEmbedding(embed_size=4, field_sizes=fs)
    assert fa.num_fields == 4 and len(fa) == 4 and len(fa.embeddings) == 4
    s = SingleIndexEmbedding(embed_size=6, field_size=9, padding_idx=0)
    assert len(s) == 6 and s.embedding.padding_idx == 0
    pre = nn.Parameter(torch.randn(5, 3, names=("N", "E")))
    s2 = SingleIndexEmbedding(embed_size=None, field_size=None, nn_embedding=pre)
    assert len(s2) == 3 and tuple(s2.embedding.weight.shape) == (5, 3)
    m.set_schema("a")
    assert m.schema.inputs == ["a"]
    with pytest.raises(ValueError):
        MultiIndicesEmbedding()
    with pytest.raises(NotImplementedError):
        MultiIndicesEmbedding(embed_size=4, field_sizes=[2, 2], sparse=True)


def test_layer_surface():
    from torecsys_amd import layers as L
    assert L.FMLayer is L.FactorizationMachineLayer and L.FFMLayer is L.FieldAwareFactorizationMachineLayer
    assert L.CINLayer is L.CompressInteractionNetworkLayer and L.DNNLayer is L.MultilayerPerceptionLayer
    assert L.FactorizationMachineLayer(None).dropout.p == 0.0            # Q1: None -> 0.0
    assert L.FactorizationMachineLayer().inputs_size == {"inputs": ("B", "N", "E")}
    assert L.InnerProductNetworkLayer(4).row_idx.tolist() == [0, 0, 0, 1, 1, 2]
    cin = L.CompressInteractionNetworkLayer(embed_size=8, num_fields=5, output_size=2, layer_sizes=[4, 6, 3])
    assert [s.Conv1d.out_channels for s in cin.model] == [8, 12, 6]      # every layer is split (quirk Q5)
    assert [s.Conv1d.in_channels for s in cin.model] == [25, 20, 30] and cin.fc.in_features == 13
    cd = L.CompressInteractionNetworkLayer(embed_size=8, num_fields=5, output_size=2, layer_sizes=[4, 6], is_direct=True)
    assert [s.Conv1d.out_channels for s in cd.model] == [4, 6]
    with pytest.raises(ValueError):
        L.MultilayerPerceptionLayer(8, 1, [4, 4], dropout_p=[0.1])


def test_no_cpu_fallback():
    from torecsys_amd import layers as L
    from torecsys_amd.inputs import MultiIndicesEmbedding
    x = torch.randn(2, 3, 4)
    for lay, inp in ((L.FMLayer(), x), (L.InnerProductNetworkLayer(3), x), (L.CrossNetworkLayer(4, 1), x),
                     (L.FFMLayer(2), torch.randn(2, 4, 4)),
                     (L.CINLayer(4, 3, 1, [2]), x)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            lay(inp)
    with pytest.raises(RuntimeError, match="no CPU path"):
        MultiIndicesEmbedding(embed_size=4, field_sizes=[2, 2])(torch.zeros(1, 2, dtype=torch.long))


def test_inputs_router_cpu_plumbing():
    """Inputs routes dict columns into (B,N) index blocks (inputs.py:69-87); checked with a recording stub."""
    from torecsys_amd.inputs import BaseInput, Inputs

    class Rec(BaseInput):
        def __init__(self):
            super().__init__()
            self.length = 1
            self.seen = None

        def forward(self, t):
            self.seen = t
            return t

    r = Rec()
    r.set_schema(["a", "b", "c"])
    out = Inputs({"x": r})({"a": torch.tensor([1, 2]), "b": torch.tensor([[3], [4]]), "c": torch.tensor([5, 6])})
    assert out["x"].tolist() == [[1, 3, 5], [2, 4, 6]]
    inp = Inputs(None)
    inp.add_inputs("y", Rec())
    with pytest.raises(AssertionError):
        inp.add_inputs("y", Rec())
    with pytest.raises(TypeError):
        inp.add_inputs(1, Rec())


def test_patch_rebinds_reference_aliases():
    import torecsys_amd
    from torecsys_amd import layers as L
    pkg = types.ModuleType("fake_trs")
    lay = types.ModuleType("fake_trs.layers")
    mdl = types.ModuleType("fake_trs.models")
    inp = types.ModuleType("fake_trs.inputs")

    class Old:  # stand-in for the reference classes
        pass
    lay.FMLayer = lay.FactorizationMachineLayer = lay.CINLayer = Old
    lay.DNNLayer = Old
    mdl.FMLayer = Old                       # `from torecsys.layers import FMLayer` inside a model module
    inp.MultiIndicesEmbedding = Old
    for m in (pkg, lay, mdl, inp):
        sys.modules[m.__name__] = m
    try:
        torecsys_amd.patch(pkg)
        assert lay.FMLayer is L.FMLayer and mdl.FMLayer is L.FMLayer and lay.CINLayer is L.CINLayer
        assert lay.DNNLayer is L.MultilayerPerceptionLayer      # the models' deep branch
        assert inp.MultiIndicesEmbedding is torecsys_amd.inputs.MultiIndicesEmbedding
        torecsys_amd.unpatch()
        assert lay.FMLayer is Old and mdl.FMLayer is Old and inp.MultiIndicesEmbedding is Old and lay.DNNLayer is Old
    finally:
        for m in (pkg, lay, mdl, inp):
            sys.modules.pop(m.__name__, None)


def test_split_count_rules():
    """split-K slice count of the MLP weight gradients (layers._split_count): divides the rows, at least 4 slices of
    at least ``slice_rows`` rows, never more than 384"""
    from torecsys_amd.layers import _split_count
    assert _split_count(65536, 2048) == 32 and _split_count(65536, 4096) == 16
    assert _split_count(16384, 2048) == 8 and _split_count(8192, 2048) == 4
    assert _split_count(4096, 2048) == 0                     # fewer than 4 slices: do not split
    for rows in (65536 * 39, 8192 * 39, 65536 * 39 // 3, 3 * 2 ** 20):
        s = _split_count(rows, 2048)
        assert 4 <= s <= 384 and rows % s == 0 and rows // s >= 2048
    assert _split_count(1000003, 2048) == 0                  # a prime row count cannot be cut evenly


def test_rowdot_width_rule():
    from torecsys_amd.functional import rowdot_width_supported
    assert rowdot_width_supported(512, 2) and rowdot_width_supported(8, 2) and rowdot_width_supported(128, 4)
    assert not rowdot_width_supported(400, 2)                # 50 vectors: not a power of two
    assert not rowdot_width_supported(1024, 2)               # 128 vectors: more than a wavefront
    assert not rowdot_width_supported(12, 2)                 # not a multiple of 16 bytes


def test_fused_optimizer_state_dict_roundtrip():
    """FusedSparse* state is keyed by the nn.Parameter, follows it across devices and survives a checkpoint
    (a resume silently reset accumulators / moments / step counts)."""
    import torch.nn as nn
    from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseAdam
    p = nn.Parameter(torch.zeros(5, 4))
    ada = FusedSparseAdagrad(0.1, initial_accumulator_value=0.5)
    st = ada.state_for(p.data, p)
    assert st.shape == (5, 4) and float(st[0, 0]) == 0.5
    st.add_(1.0)
    assert ada.state_for(p.data, p) is st                       # same parameter -> same state, new .data tensor or not
    sd = ada.state_dict([("emb.embedding.weight", p)])
    assert list(sd["tables"]) == ["emb.embedding.weight"]
    p2 = nn.Parameter(torch.zeros(5, 4))
    ada2 = FusedSparseAdagrad(0.7)
    ada2.load_state_dict(sd, [("emb.embedding.weight", p2)])
    assert ada2.lr == 0.1 and torch.equal(ada2.state_for(p2.data, p2), st)
    adam = FusedSparseAdam(1e-3)
    for _ in range(3):
        adam.next_step_size(p.data, p)
    adam.state_for(p.data, p)[0].fill_(2.0)
    sd = adam.state_dict([("w", p)])
    adam2 = FusedSparseAdam(1e-3)
    adam2.load_state_dict(sd, {"w": p2}.items())
    assert abs(adam2.next_step_size(p2.data, p2) - adam.next_step_size(p.data, p)) < 1e-12      # both at step 4
    assert torch.equal(adam2.state_for(p2.data, p2)[0], adam.state_for(p.data, p)[0])
    with pytest.raises(KeyError):
        FusedSparseAdam().load_state_dict(sd, [("other", p2)])


STANDIN = "trs_standin"       # a package laid out like torecsys: layers / inputs modules, models that import layers by name

_STANDIN_MODELS_SRC = '''
import torch
import torch.nn as nn


class FactorizationMachineModel(nn.Module):
    def __init__(self, use_bias=True, dropout_p=None):
        super().__init__()
        self.use_bias = use_bias
        self.fm = FMLayer(dropout_p)
        self.bias = nn.Parameter(torch.empty(1, 1).uniform_()) if use_bias else None

    def forward(self, feat_inputs, emb_inputs):
        emb_inputs.names = ("B", "N", "E")                    # in-place renaming of the incoming block
        first = feat_inputs.flatten(("N", "E"), "O").sum("O", keepdim=True).rename(None)
        out = self.fm(emb_inputs).rename(None).sum(dim=1, keepdim=True) + first
        return out + self.bias if self.use_bias else out


class DeepFactorizationMachineModel(nn.Module):
    def __init__(self, embed_size, num_fields, deep_layer_sizes, fm_dropout_p=None, deep_dropout_p=None):
        super().__init__()
        self.fm = FMLayer(fm_dropout_p)
        self.deep = DNNLayer(inputs_size=num_fields * embed_size, output_size=1, layer_sizes=deep_layer_sizes,
                             dropout_p=deep_dropout_p, activation=nn.ReLU())

    def forward(self, feat_inputs, emb_inputs):
        emb_inputs.names = ("B", "N", "E")
        first = feat_inputs.flatten(("N", "E"), "O").sum("O", keepdim=True).rename(None)
        fm = self.fm(emb_inputs).rename(None).sum(dim=1, keepdim=True)
        deep = self.deep(emb_inputs.flatten(("N", "E"), "E"))
        return (deep.rename(None) if deep.has_names() else deep) + fm + first


class DeepAndCrossNetworkModel(nn.Module):
    def __init__(self, inputs_size, num_fields, deep_output_size, deep_layer_sizes, cross_num_layers, output_size=1):
        super().__init__()
        self.cross = CrossNetworkLayer(inputs_size=inputs_size, num_layers=cross_num_layers)
        self.deep = DNNLayer(inputs_size=inputs_size, output_size=deep_output_size, layer_sizes=deep_layer_sizes,
                             activation=nn.ReLU())
        self.fc = nn.Linear(num_fields * (inputs_size + deep_output_size), output_size)

    def forward(self, emb_inputs):
        both = torch.cat((self.cross(emb_inputs).rename(None), self.deep(emb_inputs).rename(None)), dim=2)
        return self.fc(both.reshape(both.shape[0], -1))


class XDeepFactorizationMachineModel(nn.Module):
    def __init__(self, embed_size, num_fields, cin_layer_sizes, deep_layer_sizes):
        super().__init__()
        self.cin = CINLayer(embed_size=embed_size, num_fields=num_fields, output_size=1, layer_sizes=cin_layer_sizes,
                            is_direct=False, use_bias=True, use_batchnorm=True, activation=nn.ReLU())
        self.deep = DNNLayer(inputs_size=embed_size * num_fields, output_size=1, layer_sizes=deep_layer_sizes,
                             activation=nn.ReLU())
        self.bias = nn.Parameter(torch.empty(1).uniform_())

    def forward(self, feat_inputs, emb_inputs):
        first = feat_inputs.flatten(("N", "E"), "O").sum("O", keepdim=True).rename(None)
        deep = self.deep(emb_inputs.flatten(("N", "E"), "E"))
        return self.cin(emb_inputs).rename(None) + deep.rename(None) + first + self.bias
'''


def _standin_layer(name, dropin):
    """a stand-in layer class: same constructor and parameter layout (hence state_dict keys) as the drop-in, but a class
    of the stand-in package, not a torecsys_amd one"""
    def __init__(self, *args, **kwargs):
        nn.Module.__init__(self)
        proto = dropin(*args, **kwargs)
        for n, c in proto.named_children():
            self.add_module(n, c)
        for n, p in proto.named_parameters(recurse=False):
            self.register_parameter(n, p)
        for n, b in proto.named_buffers(recurse=False):
            self.register_buffer(n, b)
    return type(name, (nn.Module,), {"__init__": __init__, "__module__": STANDIN + ".layers"})


def _build_standin_package():
    """``trs_standin``: ``.layers`` holds every class name patch() rebinds (aliases share one class, as in torecsys),
    ``.inputs`` the three index embeddings and the ``Inputs`` router, ``.models`` four CTR models whose module holds
    ``from .layers import ...`` copies of the names and whose forwards do named-tensor plumbing of their own."""
    from torecsys_amd import inputs as I, layers as L
    from torecsys_amd import patching as P
    pkg, lay, inp, mdl = (types.ModuleType(STANDIN + s) for s in ("", ".layers", ".inputs", ".models"))
    seen = {}
    for n in P._LAYER_NAMES + P._MLP_NAMES:
        dropin = getattr(L, n)
        if dropin not in seen:
            seen[dropin] = _standin_layer(dropin.__name__, dropin)
        setattr(lay, n, seen[dropin])

    class MultiIndicesEmbedding(nn.Module):
        def __init__(self, embed_size, field_sizes):
            super().__init__()
            self.fuse_fm = False
            self.embedding = nn.Embedding(sum(field_sizes), embed_size)

        def set_schema(self, inputs):
            self.schema = list(inputs)

    class Inputs(nn.Module):
        def __init__(self, schema):
            super().__init__()
            for k, m in schema.items():
                self.add_module(k, m)

    for c in (MultiIndicesEmbedding, Inputs):
        c.__module__ = STANDIN + ".inputs"
    inp.MultiIndicesEmbedding, inp.Inputs = MultiIndicesEmbedding, Inputs
    inp.SingleIndexEmbedding = _standin_layer("SingleIndexEmbedding", I.SingleIndexEmbedding)
    inp.MultiIndicesFieldAwareEmbedding = _standin_layer("MultiIndicesFieldAwareEmbedding", I.MultiIndicesFieldAwareEmbedding)
    for n in ("FMLayer", "DNNLayer", "CrossNetworkLayer", "CINLayer"):
        setattr(mdl, n, getattr(lay, n))          # `from torecsys.layers import FMLayer, DNNLayer` in a model module
    mdl.__dict__["__name__"] = mdl.__name__
    exec(_STANDIN_MODELS_SRC, mdl.__dict__)
    pkg.layers, pkg.inputs, pkg.models = lay, inp, mdl
    return pkg, lay, inp, mdl


@pytest.fixture
def standin_pkg():
    import torecsys_amd
    mods = _build_standin_package()
    saved = {m.__name__: sys.modules.get(m.__name__) for m in mods}
    for m in mods:
        sys.modules[m.__name__] = m
    try:
        yield mods
    finally:
        torecsys_amd.unpatch()
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _build_standin_models(lay, inp, mdl, N, E, sizes):
    mods = {
        "fm": mdl.FactorizationMachineModel(use_bias=True, dropout_p=0.0),
        "deepfm": mdl.DeepFactorizationMachineModel(embed_size=E, num_fields=N, deep_layer_sizes=[16, 16],
                                                    fm_dropout_p=0.0, deep_dropout_p=[0.0, 0.0]),
        "dcn": mdl.DeepAndCrossNetworkModel(inputs_size=E, num_fields=N, deep_output_size=4, deep_layer_sizes=[16, 16],
                                            cross_num_layers=3),
        "xdeepfm": mdl.XDeepFactorizationMachineModel(embed_size=E, num_fields=N, cin_layer_sizes=[6, 6],
                                                      deep_layer_sizes=[16, 16]),
    }
    emb = inp.MultiIndicesEmbedding(embed_size=E, field_sizes=sizes)
    feat = inp.MultiIndicesEmbedding(embed_size=1, field_sizes=sizes)
    emb.set_schema(["c%d" % i for i in range(N)])
    feat.set_schema(["c%d" % i for i in range(N)])
    router = inp.Inputs(schema={"feat_inputs": feat, "emb_inputs": emb})
    return mods, emb, router


def test_patch_on_a_standin_package(standin_pkg):
    """patch() / unpatch() on a package laid out like torecsys: every hot-path name of the layers and inputs modules and
    the `from ... import` copies inside the models module are rebound (the MLP aliases included), the models built
    afterwards hold torecsys_amd classes for every hot-path child with unchanged state_dict keys and load a checkpoint of
    the un-patched models, the models' forwards are wrapped with the one-kernel heads, the router is rebound and a
    patched MultiIndicesEmbedding fuses the FM term by default; the mlp / router / fuse_fm / heads opt-outs hold and
    unpatch() restores every name, every forward and inputs.DEFAULT_FUSE_FM."""
    import warnings
    import torecsys_amd
    from torecsys_amd import inputs as I, layers as L
    from torecsys_amd import patching as P
    warnings.filterwarnings("ignore")
    pkg, lay, inp, mdl = standin_pkg
    N, E, sizes = 5, 8, [7, 3, 11, 5, 9]
    orig_names = {(m.__name__, n): getattr(m, n) for m in (lay, inp, mdl) for n in list(vars(m))
                  if n in P._LAYER_NAMES + P._MLP_NAMES + P._INPUT_NAMES + P._ROUTER_NAMES}
    model_classes = [getattr(mdl, n) for n in P._HEADS]
    orig_forwards = {c: c.__dict__["forward"] for c in model_classes}
    fuse_default = I.DEFAULT_FUSE_FM

    ref_mods, ref_emb, ref_router = _build_standin_models(lay, inp, mdl, N, E, sizes)
    ref_keys = {k: list(m.state_dict().keys()) for k, m in ref_mods.items()}
    ref_router_keys = list(ref_router.state_dict().keys())
    assert type(ref_mods["deepfm"].deep).__module__ == STANDIN + ".layers"

    assert torecsys_amd.patch(pkg) is pkg
    try:
        for (mod_name, n), old in orig_names.items():
            new = getattr(sys.modules[mod_name], n)
            assert new is not old and new is getattr(I if n in P._INPUT_NAMES + P._ROUTER_NAMES else L, n), (mod_name, n)
        for alias in P._MLP_NAMES:
            assert getattr(lay, alias) is L.MultilayerPerceptionLayer, alias
        assert mdl.DNNLayer is L.MultilayerPerceptionLayer and mdl.CrossNetworkLayer is L.CrossNetworkLayer
        assert I.DEFAULT_FUSE_FM is True
        for c in model_classes:
            assert getattr(c.__dict__["forward"], "_trs_head", False), c
        mods, emb, router = _build_standin_models(lay, inp, mdl, N, E, sizes)
        assert isinstance(mods["fm"].fm, L.FactorizationMachineLayer)
        assert isinstance(mods["deepfm"].fm, L.FactorizationMachineLayer)
        assert isinstance(mods["deepfm"].deep, L.MultilayerPerceptionLayer)
        assert isinstance(mods["dcn"].cross, L.CrossNetworkLayer)
        assert isinstance(mods["dcn"].deep, L.MultilayerPerceptionLayer)
        assert isinstance(mods["xdeepfm"].cin, L.CompressInteractionNetworkLayer)
        assert isinstance(mods["xdeepfm"].deep, L.MultilayerPerceptionLayer)
        assert isinstance(emb, I.MultiIndicesEmbedding) and emb.fuse_fm is True
        assert isinstance(router, I.Inputs)
        for k, m in mods.items():
            assert list(m.state_dict().keys()) == ref_keys[k], k
            for c in m.modules():      # nothing of the stand-in's layer module is left inside the models
                assert not type(c).__module__.startswith(STANDIN + ".layers"), (k, type(c))
            m.load_state_dict(ref_mods[k].state_dict())
        assert list(router.state_dict().keys()) == ref_router_keys
        router.load_state_dict(ref_router.state_dict())
        assert torecsys_amd.patch(pkg) is pkg          # a second patch() changes nothing
        assert lay.FMLayer is L.FMLayer and getattr(mdl.DeepFactorizationMachineModel.forward, "_trs_head", False)
    finally:
        torecsys_amd.unpatch()
    for (mod_name, n), old in orig_names.items():
        assert getattr(sys.modules[mod_name], n) is old, (mod_name, n)
    for c in model_classes:
        assert c.__dict__["forward"] is orig_forwards[c], c
    assert I.DEFAULT_FUSE_FM is fuse_default is False

    # opt-outs
    torecsys_amd.patch(pkg, fuse_fm=False, mlp=False, router=False, heads=False)
    try:
        m2, e2, r2 = _build_standin_models(lay, inp, mdl, N, E, sizes)
        assert isinstance(e2, I.MultiIndicesEmbedding) and e2.fuse_fm is False and I.DEFAULT_FUSE_FM is False
        assert not isinstance(r2, I.Inputs) and inp.Inputs is orig_names[(inp.__name__, "Inputs")]
        assert not isinstance(m2["deepfm"].deep, L.MultilayerPerceptionLayer)
        assert all(getattr(lay, a) is orig_names[(lay.__name__, a)] for a in P._MLP_NAMES)
        assert isinstance(m2["deepfm"].fm, L.FactorizationMachineLayer) and isinstance(m2["dcn"].cross, L.CrossNetworkLayer)
        for c in model_classes:
            assert c.__dict__["forward"] is orig_forwards[c], c
    finally:
        torecsys_amd.unpatch()
    m3, e3, r3 = _build_standin_models(lay, inp, mdl, N, E, sizes)
    assert type(m3["deepfm"].fm).__module__ == STANDIN + ".layers" and not isinstance(e3, I.MultiIndicesEmbedding)
    assert not isinstance(r3, I.Inputs)


def _install_cpu_standins(monkeypatch):
    """torch-CPU statements of the functional entry points the four models' drop-in modules reach, backed by the oracle
    (TEST ONLY: the product entry points are HIP kernels and refuse CPU tensors).  They keep the product's calling
    conventions -- return values, the (B,E) FM side output, the (B,C,E) contraction layout -- so that everything ABOVE
    them (the drop-in modules' forwards, the named-tensor plumbing of the reference's own model code) runs unchanged."""
    from oracle import cpu_ref as O
    from torecsys_amd import functional as F_
    calls = {"embed_fm": 0, "fm_layer": 0, "cross_network": 0, "cin_contract": 0, "gather_rows": 0}

    def _idx(idx):
        idx = idx.rename(None) if idx.has_names() else idx
        return idx.unsqueeze(-1) if idx.dim() == 1 else idx

    def embed_fm(weight, idx, offsets=None, first_weight=None, want_emb=True, opt=None, padding_idx=None):
        calls["embed_fm"] += 1
        emb = O.multi_indices_embedding(weight, _idx(idx), offsets)
        first = None if first_weight is None else O.multi_indices_embedding(first_weight, _idx(idx), offsets).sum(dim=1)
        return (emb if want_emb else None), O.fm_layer(emb), first

    def gather_rows(weight, idx, offsets=None, padding_idx=None, opt=None):
        calls["gather_rows"] += 1
        if offsets is None:
            return O.single_index_embedding(weight, _idx(idx), padding_idx)
        return O.multi_indices_embedding(weight, _idx(idx), offsets)

    def fm_layer(x):
        calls["fm_layer"] += 1
        return O.fm_layer(x)

    def cross_network(x, W, b, detach_first=True):
        calls["cross_network"] += 1
        return O.cross_network(x, list(W), list(b), detach_first)

    def cin_contract(x0, xk, Wc, bias):
        calls["cin_contract"] += 1
        return O.cin_contraction(x0.transpose(1, 2), xk.transpose(1, 2), Wc.unsqueeze(-1), bias)

    for name, fn in [("embed_fm", embed_fm), ("gather_rows", gather_rows), ("fm_layer", fm_layer),
                     ("cross_network", cross_network), ("cin_contract", cin_contract),
                     ("prefetch_row_buckets", lambda *a, **k: None)]:
        monkeypatch.setattr(F_, name, fn)
    return calls


def test_standin_model_forwards_carry_the_fused_fm_term(standin_pkg, monkeypatch):
    """Model code of the user's package drives the drop-ins: after ``patch()``, the stand-in FM / DeepFM models' own
    forwards -- named-tensor plumbing on the blocks that come out of this package's lookups (in-place
    ``emb_inputs.names = ...``, ``flatten(('N', 'E'), ...)``, ``sum('O')``) -- run forward + backward through ``Inputs``.
    The HIP entry points are replaced by oracle-backed CPU stand-ins inside this test only.  Checked: the fused FM term
    rides from the lookup to FMLayer through the renaming (one fused lookup per wide-table pass and NOT ONE separate FM
    pass); logits and the table gradients equal the oracle models on the same parameters; with fuse_fm off the FM
    layer runs its own pass and the logits are the same."""
    import warnings
    import torecsys_amd
    warnings.filterwarnings("ignore")
    pkg, lay, inp, mdl = standin_pkg
    B, N, E, sizes = 6, 5, 8, [7, 3, 11, 5, 9]
    g = torch.Generator().manual_seed(3)
    cols = {"c%d" % i: torch.randint(0, sizes[i], (B,), generator=g) for i in range(N)}
    idx = torch.stack([cols["c%d" % i] for i in range(N)], dim=1)
    off = O.field_offsets(sizes)

    def run(fuse_fm):
        torecsys_amd.patch(pkg, fuse_fm=fuse_fm)
        try:
            calls = _install_cpu_standins(monkeypatch)
            torch.manual_seed(5)
            mods, _, router = _build_standin_models(lay, inp, mdl, N, E, sizes)
            out = {}
            for k in ("fm", "deepfm"):
                m = mods[k]
                for p in list(router.parameters()) + list(m.parameters()):
                    p.grad = None
                d = router({c: v.clone() for c, v in cols.items()})
                y = m(**d)
                assert tuple(y.shape) == (B, 1) and not y.has_names(), (k, y.names)
                y.sum().backward()
                sd = {n: p.detach() for n, p in m.named_parameters()}
                w, w1 = router.emb_inputs.embedding.weight, router.feat_inputs.embedding.weight
                wr, w1r = w.detach().clone().requires_grad_(), w1.detach().clone().requires_grad_()
                emb, feat = O.multi_indices_embedding(wr, idx, off), O.multi_indices_embedding(w1r, idx, off)
                if k == "fm":
                    ref = O.fm_model(feat, emb, sd["bias"])
                else:
                    names = [n[:-len(".weight")] for n in sd if n.startswith("deep.") and n.endswith(".weight")]
                    ref = O.deepfm_model(feat, emb, [sd[n + ".weight"] for n in names], [sd[n + ".bias"] for n in names])
                ref.sum().backward()
                assert float((y.detach() - ref.detach()).abs().max()) <= 1e-5 * float(ref.abs().max()), k
                for got, want in ((w.grad, wr.grad), (w1.grad, w1r.grad)):
                    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), k
                out[k] = y.detach()
            return out, calls
        finally:
            torecsys_amd.unpatch()

    fused, calls = run(True)
    # two wide-table lookups (one per model), each fused with the FM term, and no separate FM pass
    assert calls["embed_fm"] == 2 and calls["gather_rows"] == 2 and calls["fm_layer"] == 0, calls
    plain, calls2 = run(False)
    assert calls2["embed_fm"] == 0 and calls2["fm_layer"] == 2, calls2
    for k in fused:
        assert torch.allclose(fused[k], plain[k], rtol=1e-5, atol=1e-6), k


@pytest.mark.parametrize("N", [2, 3, 7, 16, 32, 33, 39, 40, 48])
def test_afm_pair_tiles_cover_every_pair_once_and_are_field_disjoint(N):
    """the host-built tile schedule of the AFM backward kernel (afm_packed_tiles): each of the N(N-1)/2 pairs exactly once,
    no field twice inside a tile, and no more tiles than the round-robin rounds would take"""
    import ctypes
    import numpy as np
    from torecsys_amd import _abi
    lib = _abi.load()
    buf = np.full(112 * 16, 0xffff, dtype=np.uint16)
    nt = ctypes.c_int32(0)
    rc = lib.trs_afm_pair_tiles(N, buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(nt))
    assert rc == 0 and nt.value > 0
    seen = set()
    for t in range(nt.value):
        fields = set()
        for e in buf[16 * t:16 * t + 16]:
            if e == 0xffff:
                continue
            i, j = int(e) >> 8, int(e) & 0xff
            assert 0 <= i < j < N
            assert (i, j) not in seen
            seen.add((i, j))
            assert i not in fields and j not in fields
            fields.update((i, j))
    assert len(seen) == N * (N - 1) // 2
    assert np.all(buf[16 * nt.value:] == 0xffff)
    rounds = N if N % 2 else N - 1
    assert nt.value <= rounds * ((N // 2 + 15) // 16)
    if N > 32:
        assert nt.value == -(-len(seen) // 16)          # the greedy pass reaches the lower bound for these N


@pytest.mark.parametrize("N,C,E", [(5, 4, 3), (33, 8, 4), (39, 6, 2)])
def test_cin_symmetric_fold_keeps_the_first_layer_contraction(N, C, E):
    """functional.cin_fold_symmetric: with xk = x0 the oracle's contraction gives the same (B,C,E) for the folded weights
    (and their gradient w.r.t. x0, which is what the data-gradient kernel returns as dx0 + dxk), in float64"""
    from torecsys_amd import functional as F_
    from oracle import cpu_ref as O
    g = torch.Generator().manual_seed(N)
    x = torch.randn(3, E, N, generator=g, dtype=torch.float64)
    W = torch.randn(C, N * N, generator=g, dtype=torch.float64)
    Wf = F_.cin_fold_symmetric(W.float(), N).double()
    # exactness of the fold itself is a property of real arithmetic: redo it in float64 for the comparison
    W3 = W.view(C, N, N)
    Wf64 = (torch.tril(W3) + torch.triu(W3, 1).transpose(1, 2)).reshape(C, N * N)
    assert float((Wf - Wf64).abs().max()) <= 1e-6 * float(W.abs().max()) * 2
    assert float(torch.triu(Wf64.view(C, N, N), 1).abs().max()) == 0.0
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya = O.cin_contraction(xa, xa, W.unsqueeze(-1), None)
    yb = O.cin_contraction(xb, xb, Wf64.unsqueeze(-1), None)
    assert float((ya - yb).abs().max()) <= 1e-10 * float(ya.abs().max())
    go = torch.randn(ya.shape, generator=g, dtype=torch.float64)
    (ya * go).sum().backward()
    (yb * go).sum().backward()
    assert float((xa.grad - xb.grad).abs().max()) <= 1e-10 * float(xa.grad.abs().max())


# kernel-name prefix -> (most VGPRs it may spill, why it is tolerated).  Everything else in csrc/ must not spill at all:
# scratch traffic in a hot loop is the first thing a review of these kernels looks for.
SPILL_ALLOWLIST = {
    "void trs::cin_cl_bwd_data_kernel<4, 4, 3, 8>": (2, "two address registers saved once per item, outside the k-loops"),
    "void trs::cross_mfma_bwd3_kernel<4, 6, false>": (10, "the NON-detached variant (faithful_grad=False) keeps one more "
                                                          "packed gradient tile; the default variant <4, 6, true> has none"),
    "trs::mlp_fused_fwd_kernel": (10, "kernel-invariant addresses saved at entry and re-read once per tile / layer "
                                      "(profiles/r04_kernels.md); none inside a k-loop"),
    "void trs::mlp_fused_bwd_kernel<true>": (5, "the variant that reads the row-owner sign bits: five kernel-invariant values "
                                                "stored once at entry, six single reloads per tile between the GEMM variants, "
                                                "none inside a k-loop (11 scratch instructions in 11.7 k lines of ISA)"),
    "void trs::pairw_reg_kernel<float, 1>": (13, "OPN 'vec' weight gradient: 64 accumulators per lane at the 128-register "
                                                 "cap of a 1024-thread workgroup (one pair per lane needs the 1024 threads)"),
    "void trs::pairw_reg_kernel<trs::bf16_t, 1>": (12, "as above"),
    "void trs::mlp_ro_kernel<trs::RoCfg<416, 400, 400, 8>, false, 416, 1>": (1, "one per-pass value saved at the start of a "
                                                                               "pass and re-read once at its end (the 416-wide "
                                                                               "input takes 104 of the 256 registers)"),
}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_unexpected_register_spills():
    """hipcc's own resource report over every file of csrc/ (the build's flags): no kernel that can be dispatched spills
    VGPRs, beyond a short allowlist whose entries say why.  Last round shipped never-selected template instantiations
    that spilled up to 589 registers and a hot kernel that had quietly grown scratch traffic."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spills
    bad = spills.spilling_kernels()
    unexpected = []
    for src, name, vs, ss, v, a in bad:
        lim = SPILL_ALLOWLIST.get(name)
        if lim is None or vs > lim[0]:
            unexpected.append((src, name, vs))
    assert not unexpected, f"kernels with VGPR spills: {unexpected}"


def test_bench_self_launches_for_more_than_one_gpu(monkeypatch):
    """`python bench.py --gpus N` (the driver's BENCH command form, no launcher around it) must start N ranks by itself:
    the process replaces itself with torch.distributed.run on 127.0.0.1; under a launcher (WORLD_SIZE set) or at N = 1
    it does not."""
    import importlib.util
    monkeypatch.setattr(sys, "argv", ["bench.py", "--no-tunableop"])       # module import must not touch TunableOp files
    spec = importlib.util.spec_from_file_location("trs_bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    argv = ["bench.py", "--gpus", "8", "--steps", "20", "--warmup", "5"]
    cmd = bench.self_launch_argv(8, argv, {})
    assert cmd[0] == sys.executable and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    i = cmd.index(os.path.join(ROOT, "bench.py")) if os.path.join(ROOT, "bench.py") in cmd else cmd.index(os.path.abspath("bench.py"))
    assert cmd[i + 1:] == argv[1:]
    assert bench.self_launch_argv(8, argv, {"MASTER_PORT": "29777"})[cmd.index("--master-port") + 1] == "29777"
    assert bench.self_launch_argv(8, argv, {"WORLD_SIZE": "8", "RANK": "0"}) is None
    assert bench.self_launch_argv(1, argv, {}) is None
    # main() execs exactly that command
    seen = {}

    def fake_execv(path, args):
        seen["path"], seen["args"] = path, list(args)
        raise SystemExit(0)

    monkeypatch.setattr(os, "execv", fake_execv)
    monkeypatch.setattr(sys, "argv", [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--no-tunableop"])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit):
        bench.main()
    assert seen["path"] == sys.executable and seen["args"][seen["args"].index("--nproc-per-node") + 1] == "2"
    assert seen["args"][-5:] == ["--gpus", "2", "--steps", "4", "--no-tunableop"]


def _load_bench(monkeypatch):
    import importlib.util
    monkeypatch.setattr(sys, "argv", ["bench.py", "--no-tunableop"])       # module import must not touch TunableOp files
    spec = importlib.util.spec_from_file_location("trs_bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_plain_run_leaves_the_extra_legs_to_full(monkeypatch):
    """a plain `bench.py` run measures the headline only: every extra leg is off unless --full is given, and under --full
    the --no-* options still opt out of single legs"""
    bench = _load_bench(monkeypatch)
    legs = ("no_cpu_baseline", "no_large_table", "no_other_models", "no_variants")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert not a.full and a.steps == 7 and a.warmup == 3 and a.dump_outputs is None
    assert all(getattr(a, k) for k in legs)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out" and not any(getattr(a, k) for k in legs)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.no_cpu_baseline and not (a.no_large_table or a.no_other_models or a.no_variants)


def test_bench_dump_outputs(monkeypatch, tmp_path):
    """--dump-outputs: loss and gradients as float32 .npy; a tensor above DUMP_WHOLE_MAX elements -- dense, or the sparse
    COO gradient of a large row-sharded table -- is cut to the same seeded rows in every call; 64 MB at most"""
    import numpy as np
    bench = _load_bench(monkeypatch)

    class P:
        def __init__(self, grad):
            self.grad = grad

    V, E = 1_000_000, 64
    g = torch.Generator().manual_seed(1)
    big = torch.randn(V, E, generator=g).to(torch.bfloat16)
    ids = torch.randint(0, 20_000_000, (200_000,), generator=g)
    sp = torch.sparse_coo_tensor(ids.unsqueeze(0), torch.randn(200_000, 4, generator=g), size=(20_000_000, 4))
    small_sp = torch.sparse_coo_tensor(torch.tensor([[1, 1, 5]]), torch.ones(3, 3), size=(100, 3))
    named = [("emb", P(big)), ("shard", P(sp)), ("small", P(small_sp)), ("w", P(torch.randn(400, 400, generator=g))),
             ("frozen", P(None))]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(0.25), named, False)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["grad.emb.npy", "grad.shard.npy", "grad.small.npy", "grad.w.npy", "loss.npy"]
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and np.array_equal(x, y), f
    rows = torch.randint(0, V, (bench.DUMP_SAMPLE_ROWS,), generator=torch.Generator().manual_seed(0)).sort().values
    assert np.array_equal(np.load(tmp_path / "a" / "grad.emb.npy"), big[rows].float().numpy())
    rows = torch.randint(0, 20_000_000, (bench.DUMP_SAMPLE_ROWS,), generator=torch.Generator().manual_seed(0)).sort().values
    assert np.array_equal(np.load(tmp_path / "a" / "grad.shard.npy"), sp.coalesce().index_select(0, rows).to_dense().numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "grad.small.npy"), small_sp.to_dense().numpy())
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [0.25]
    # the cap: five tensors of DUMP_WHOLE_MAX fp32 elements (16 MB each) are more than 64 MB
    many = [("t%d" % i, P(torch.zeros(bench.DUMP_WHOLE_MAX))) for i in range(5)]
    with pytest.raises(AssertionError, match="dump-outputs"):
        bench.dump_outputs(str(tmp_path / "c"), torch.tensor(0.0), many, False)
