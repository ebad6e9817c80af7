"""``LocationEncoder`` for RANGE / RANGE+ on MI355X - the drop-in for the reference's
range/range.py:69-278 (RANGE branches: __init__ :76-114, forward :208-242).

Same constructor contract (an ``argparse.Namespace`` with ``location_model_name``,
``pretrained_path``, ``device``, ``range_db``, ``beta``), same attributes other code reads
(``location_feature_dim``, ``args.temp`` / ``args.geo_temp`` / ``args.beta``), same exceptions for
the same conditions, same call: ``model(coords)`` with ``coords`` a (B,2) float64 tensor of
(lon, lat) degrees returns a host ``numpy.ndarray`` (B,1280) float64.

All arithmetic runs in hand-written HIP kernels behind librange_hip.so (range_amd/_native.py);
there is no torch-op or CPU fallback.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _native, posenc
from ._hostpool import POOL
from .bank import PreparedBank
from .bankfile import load_any as load_bank
from .ckpt import EncoderParams, read_checkpoint
from .csp import ACTIVATIONS as CSP_ACTIVATIONS, CspParams, read_csp_checkpoint

TEMP_RANGE = 15.0        # range/range.py:103
TEMP_RANGE_PLUS = 12.0   # range/range.py:108
TEMP_GEO = 40.0          # range/range.py:109

# training-free coordinate encoders: load_model name -> (kernel mode, the reference's banner)
_COORD_MODELS = {
    "Direct": (_native.COORD_DIRECT, "Using Direct Encoding"),          # range.py:153-156
    "Cartesian_3D": (_native.COORD_CARTESIAN3D, "Using Cartesian_3D"),   # range.py:159-162
    "Wrap": (_native.COORD_WRAP, "Using Wrap"),                          # range.py:170-173
}


def _device_of(spec) -> torch.device:
    dev = torch.device(spec)
    if dev.type != "cuda":
        raise RuntimeError(
            f"range_amd runs on MI355X GPUs only (device={spec!r}); there is no CPU path. "
            "Use the reference implementation for CPU inference.")
    return dev


MAX_TEMP_CONSTANT = 43.0  # include/range_hip.h: RANGE_MAX_TAU (the constant-shift kernels)
MAX_TEMP = 1000.0         # RANGE_MAX_TAU_SHARP


def check_temperatures(name: str, temp, geo_temp=None, pv_mode: Optional[str] = None):
    """Validate the softmax temperatures of "RANGE" / "RANGE+" (``args.temp`` / ``args.geo_temp``; None:
    the reference's default) -> (tau_sem, tau_geo) floats, tau_geo = 0 for "RANGE".  Pure: no GPU.
    ValueError for a temperature that is not finite, not > 0 or above 1000 (there the softmax is an
    argmax to float32 precision), for ``geo_temp`` with plain "RANGE" (it has no geographic head),
    and for a temperature above 43 together with ``pv_mode='bf16x3'`` (the bf16-plane pass 2 is
    tuned and tested for the constant-shift range only)."""
    if name not in ("RANGE", "RANGE+"):
        raise ValueError("Unimplemented RANGE model")                   # range.py:113-114
    if name == "RANGE" and geo_temp is not None:
        raise ValueError("geo_temp applies to RANGE+ only: RANGE has no geographic retrieval")
    tau_sem = float(TEMP_RANGE if name == "RANGE" else TEMP_RANGE_PLUS) if temp is None else float(temp)
    tau_geo = 0.0 if name == "RANGE" else (float(TEMP_GEO) if geo_temp is None else float(geo_temp))
    for what, tau in (("temp", tau_sem),) + ((("geo_temp", tau_geo),) if name == "RANGE+" else ()):
        if not (np.isfinite(tau) and 0.0 < tau <= MAX_TEMP):
            raise ValueError(f"{what}={tau!r}: a temperature must be finite, > 0 and at most {MAX_TEMP:g}")
    if pv_mode == "bf16x3" and max(tau_sem, tau_geo) > MAX_TEMP_CONSTANT:
        raise ValueError(f"pv_mode='bf16x3' supports temperatures up to {MAX_TEMP_CONSTANT:g} "
                         f"(temp={tau_sem:g}, geo_temp={tau_geo:g}): use pv_mode='exact'")
    return tau_sem, tau_geo


def range_model(name: str, temp=None, geo_temp=None):
    """"RANGE" / "RANGE+" -> (tau_sem, tau_geo, kernel model id, the reference's banner); tau_geo = 0:
    no geographic retrieval.  ``temp`` / ``geo_temp``: other temperatures than the reference's
    defaults (``check_temperatures``)."""
    tau_sem, tau_geo = check_temperatures(name, temp, geo_temp)
    if name == "RANGE":                                                 # range.py:102-105
        return tau_sem, 0.0, _native.MODEL_RANGE, f"Using RANGE with temperature {tau_sem}"
    return (tau_sem, tau_geo, _native.MODEL_RANGE_PLUS,                 # :107-112
            f"Using RANGE+ with temperatures {tau_sem} and {tau_geo}")


def attend_any(eng, kept: bool, first: int, e32, xq, tau_sem, tau_geo, beta, stats):
    """Pass 2 for queries [first, first + len(xq)) of the last scan: from its logits when the scan
    kept them (``kept``), else recomputed from their e-hat ``e32`` - bit-identical partials."""
    if kept:
        return eng.attend_kept(first, xq, tau_sem, tau_geo, beta, stats)
    return eng.attend(e32, xq, tau_sem, tau_geo, beta, stats)


class SweepPlan:
    """What a temperature sweep runs (``sweep_plan``): the validated lists, the temperature pairs whose
    statistics it needs and the leading dimensions of its result."""

    def __init__(self, temps, geo_temps, betas, pairs, lead):
        self.temps, self.geo_temps, self.betas, self.pairs, self.lead = temps, geo_temps, betas, pairs, lead

    @property
    def scan_taus(self):
        """The temperatures of the one scan that keeps the logits: the first of each list."""
        return self.temps[0], (self.geo_temps[0] if self.geo_temps else 0.0)


def sweep_plan(name: str, betas, temps, geo_temps, args_temp, args_geo_temp=None, args_beta=None,
               pv_mode: Optional[str] = None) -> Optional[SweepPlan]:
    """The arguments of ``sweep(coords, betas, temps=, geo_temps=)`` -> a ``SweepPlan``, or None for the
    plain beta sweep (both lists None).  Pure: no GPU.

    RANGE+ with either list: a missing list is ``[args_temp]`` / ``[args_geo_temp]``, ``betas=None`` is
    ``[args_beta]``; the result is (T, G, nb, B, 1280).  RANGE with ``temps``: ``betas`` and
    ``geo_temps`` must be None; the result is (T, B, 1280).  Every value goes through
    ``check_temperatures`` (its bf16x3 rule included); an empty list is a ValueError.

    Pairs: the semantic retrieval H_i runs at (temps[i], 0) - no geographic head, what plain RANGE runs
    at that temperature - and the geographic retrieval G_j at (TEMP_RANGE_PLUS, geo_temps[j]), its
    semantic weight multiplied by beta = 0: a head's bits do not depend on what else is in the lists."""
    if temps is None and geo_temps is None:
        return None
    if name not in ("RANGE", "RANGE+"):
        raise ValueError("sweep() is defined for RANGE / RANGE+ only")
    if name == "RANGE":
        if geo_temps is not None:
            raise ValueError("geo_temps applies to RANGE+ only: RANGE has no geographic retrieval")
        if betas is not None:
            raise ValueError("betas applies to RANGE+ only: RANGE has no blend")
    ts = [args_temp] if temps is None else list(temps)
    gs = [] if name == "RANGE" else ([args_geo_temp] if geo_temps is None else list(geo_temps))
    bs = [] if name == "RANGE" else ([args_beta] if betas is None else list(betas))
    for what, lst in (("temps", ts),) + ((("geo_temps", gs), ("betas", bs)) if name == "RANGE+" else ()):
        if len(lst) == 0:
            raise ValueError(f"{what} must not be empty")
    ts = [check_temperatures(name, t, None, pv_mode)[0] for t in ts]
    gs = [check_temperatures(name, None, g, pv_mode)[1] for g in gs]
    bs = [float(b) for b in bs]
    pairs = [(t, 0.0) for t in ts] + [(float(TEMP_RANGE_PLUS), g) for g in gs]
    lead = (len(ts),) if name == "RANGE" else (len(ts), len(gs), len(bs))
    return SweepPlan(ts, gs, bs, pairs, lead)


def _as_coords(coords, device) -> torch.Tensor:
    if not torch.is_tensor(coords):
        coords = torch.as_tensor(np.asarray(coords))
    if coords.dim() != 2 or coords.shape[1] != 2:
        raise ValueError(f"coords must be (B,2) (lon,lat) degrees, got {tuple(coords.shape)}")
    # the reference requires float64 input (F.linear against .double() weights);
    # float32 input is accepted here by widening
    return coords.to(device=device, dtype=torch.float64).contiguous()


def _topk_arg(return_topk, has_bank: bool = True) -> int:
    k = int(return_topk)
    if not has_bank:
        raise ValueError("return_topk needs a bank (RANGE / RANGE+)")
    if not 1 <= k <= _native.MAX_TOPK:
        raise ValueError(f"return_topk must be in 1..{_native.MAX_TOPK}, got {return_topk}")
    return k


def _load(args, with_bank: bool):
    """The bank (``with_bank``) and the encoder checkpoint ``args`` name; both 256 wide."""
    bank = load_bank(args.range_db) if with_bank else None              # range.py:78-95
    enc = read_checkpoint(args.pretrained_path)                         # :82-84
    if enc.embed_dim != 256:
        raise ValueError(f"checkpoint embed_dim {enc.embed_dim}" +
                         (" != bank key width 256" if with_bank else ": only 256 is implemented"))
    return bank, enc


_SH_TABLES = {}     # (L, source path or None) -> SHTable


def sh_table_for(enc: EncoderParams, sh_eval: Optional[str] = None, sh_source: Optional[str] = None):
    """The coefficient table of the reference's generated "analytic" spherical harmonics, or None.

    ``sh_eval``: 'reference' (default for harmonics_calculation == 'analytic': the reference's own
    expanded polynomials with their 15-digit coefficients, so that embeddings agree with the
    reference at every latitude) or 'exact' (the stable recurrence: the mathematically exact basis,
    which the reference itself only matches for |lat| <~ 45 deg).  'closed-form' checkpoints always
    use the recurrence - it is what the reference runs for them
    (spherical_harmonics_closed_form.py:8-40).  ``sh_source``: path of a generated
    ``spherical_harmonics_ylm.py`` to take the coefficients from (default: regenerate them)."""
    if sh_eval is None:
        sh_eval = "reference"
    if sh_eval not in ("reference", "exact"):
        raise ValueError(f"sh_eval must be 'reference' or 'exact', got {sh_eval!r}")
    if enc.harmonics_calculation != "analytic" or sh_eval == "exact":
        return None
    from . import sh_table
    key = (enc.legendre_polys, sh_source)
    if key not in _SH_TABLES:
        if sh_source is not None:
            with open(sh_source) as f:
                _SH_TABLES[key] = sh_table.parse_ylm_source(f.read(), enc.legendre_polys)
        else:
            _SH_TABLES[key] = sh_table.generate_table(enc.legendre_polys)
    return _SH_TABLES[key]


def make_engine(enc: EncoderParams, bank: Optional[PreparedBank], device, row_offset: int = 0,
                sh_eval: Optional[str] = None, sh_source: Optional[str] = None,
                pv_mode: Optional[str] = None):
    """``pv_mode``: None / 'exact' (the reference's float32 products) or the opt-in 'bf16x3'
    (include/range_hip.h: range_set_pv_mode)."""
    eng = _native.HipEngine(device)
    if pv_mode is not None:
        eng.set_pv_mode(pv_mode)
    mode = _native.SH_ANALYTIC if enc.harmonics_calculation == "analytic" else _native.SH_CLOSED_FORM
    eng.set_encoder(enc.legendre_polys, enc.hidden, enc.num_hidden_layers, enc.embed_dim, mode,
                    enc.weights, enc.biases, sh_table=sh_table_for(enc, sh_eval, sh_source))
    if bank is not None:
        eng.set_bank(bank.keys, bank.values, bank.xyz, row_offset)
    return eng


class _FrozenLinear(nn.Module):
    """The parameters of one SirenNet layer (``weight`` (out,in), ``bias`` (out,) float64, frozen), under
    the reference's names (satclip/location_encoder.py:121-151)."""

    def __init__(self, weight: np.ndarray, bias: np.ndarray, device):
        super().__init__()
        self.weight = nn.Parameter(torch.as_tensor(np.asarray(weight), dtype=torch.float64, device=device), requires_grad=False)
        self.bias = nn.Parameter(torch.as_tensor(np.asarray(bias), dtype=torch.float64, device=device), requires_grad=False)


class _SirenParams(nn.Module):
    def __init__(self, enc: EncoderParams, device):
        super().__init__()
        n = enc.num_hidden_layers
        self.layers = nn.ModuleList([_FrozenLinear(enc.weights[i], enc.biases[i], device) for i in range(n)])
        self.last_layer = _FrozenLinear(enc.weights[n], enc.biases[n], device)


class SatCLIPLocationModel(nn.Module):
    """``model.loc_model`` of the reference (range/range.py:83-84, 119-121: ``get_satclip(...).double()``
    = satclip/location_encoder.py:267-275 ``LocationEncoder(posenc, nnet)``): a module whose call maps
    (B,2) float64 (lon,lat) degrees to the RAW - un-normalised - (B,256) float64 SatCLIP embedding on
    the device, and whose parameters are the SirenNet's, frozen (range.py:201-203), float64, on the
    engine's GPU, under the reference's names (``nnet.layers.{i}.weight`` ...: the checkpoint's
    ``model.location.*`` keys) - so that ``next(model.parameters()).device``, ``requires_grad`` checks,
    ``state_dict()`` and ``model.to(device)`` behave as on the reference.  The parameters are a
    read-only MIRROR: the arithmetic runs in the engine (fused HIP kernel A on its own re-packed copy of
    the same weights); writing to them does not change the model."""

    def __init__(self, engine, enc: EncoderParams, chunk_size: int = 16384):
        super().__init__()
        self.nnet = _SirenParams(enc, engine.device)
        self._engine = [engine]          # (a list: not a sub-module, not part of the state dict)
        self._chunk = chunk_size
        self.eval()

    @torch.no_grad()
    def forward(self, coords: torch.Tensor) -> torch.Tensor:
        eng = self._engine[0]
        x = _as_coords(coords, eng.device)
        if x.shape[0] == 0:
            return torch.empty((0, 256), dtype=torch.float64, device=x.device)
        parts = [eng.encode_raw(x[i:i + self._chunk]) for i in range(0, x.shape[0], self._chunk)]
        return parts[0] if len(parts) == 1 else torch.cat(parts)


class _CoordLocationModel(nn.Module):
    """``loc_model`` of the training-free encoders: the reference's ``DummyLocationEncoder`` (identity;
    'Direct', 'Cartesian_3D': range.py:155, 161) and ``Wrap()`` (:172) - parameter-free modules there
    too (``next(model.parameters())`` raises StopIteration on both sides)."""

    def __init__(self, engine, mode):
        super().__init__()
        self._engine, self._mode = [engine], mode

    @torch.no_grad()
    def forward(self, x):
        if self._mode != _native.COORD_WRAP:
            return x                                                      # DummyLocationEncoder
        eng = self._engine[0]
        x = torch.as_tensor(x).to(device=eng.device, dtype=torch.float64).contiguous()
        return eng.coord_features(x, _native.COORD_WRAP) if x.shape[0] else torch.empty((0, 4), dtype=torch.float64, device=x.device)


class PosencLocationModel(nn.Module):
    """``loc_model`` of 'Theory' (``Theory(frequency_num=32, min_radius=1)``, range.py:167) and of the
    's2vec_*' names (``get_sphere2vec(name=...)``, :180): parameter-free modules there too, with the same
    read-only attributes - ``frequency_num``, ``min_radius``, ``max_radius``, ``freq_list``,
    ``embedding_dim``, and ``name`` for the s2vec kinds.  The call maps (B,2) (lon,lat) degrees to the
    (B, embedding_dim) encoding in the coordinates' dtype, a tensor on the engine's GPU (the reference
    computes it with numpy on the host, in float64 whatever the dtype, and converts back)."""

    def __init__(self, engine, model_name: str):
        super().__init__()
        s = posenc.spec(model_name)
        self._engine, self._kind = [engine], s.kind
        self.frequency_num, self.min_radius, self.max_radius = s.frequency_num, s.min_radius, s.max_radius
        self.freq_list = posenc.freq_list(model_name)
        self.freq_list.setflags(write=False)
        self.embedding_dim = s.width
        if model_name != "Theory":
            self.name = model_name.split("_")[-1]                         # range.py:179

    @staticmethod
    def result_dtype(coords) -> torch.dtype:
        """The reference converts its float64 result to the coordinates' dtype (theory.py:90,
        sphere2vec.py:248); anything that is not a floating-point tensor / array counts as float64."""
        dt = coords.dtype if torch.is_tensor(coords) else torch.as_tensor(np.asarray(coords)).dtype
        return dt if dt.is_floating_point else torch.float64

    @torch.no_grad()
    def forward(self, coords):
        return self.encode(_as_coords(coords, self._engine[0].device), self.result_dtype(coords))

    def encode(self, x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """``x``: (B,2) float64 on the engine's GPU (the coordinates widened) -> (B, embedding_dim) ``dtype``."""
        if x.shape[0] == 0:
            return torch.empty((0, self.embedding_dim), dtype=dtype, device=x.device)
        return self._engine[0].posenc_features(x, self._kind, self.freq_list).to(dtype)


# the reference's banners (range.py:142; :148 prints a garbled 'Using CSP-IN75.97lkjhat')
_CSP_MODELS = {"CSP": "Using CSP-FMOW", "CSP_INat": "Using CSP-INat"}


class _CspLayer(nn.Module):
    """One ``SingleFeedForwardNN`` (csp/main/module.py:48-132): ``linear`` and, where the checkpoint has one,
    ``layernorm`` - float32, frozen."""

    def __init__(self, p: CspParams, i: int, device):
        super().__init__()
        frozen = lambda a: nn.Parameter(torch.as_tensor(a, dtype=torch.float32, device=device), requires_grad=False)  # noqa: E731
        d_out, d_in = p.weights[i].shape
        self.linear = nn.Linear(d_in, d_out, device="meta")
        self.linear.weight, self.linear.bias = frozen(p.weights[i]), frozen(p.biases[i])
        if p.ln_gamma[i] is not None:
            self.layernorm = nn.LayerNorm(d_out, device="meta")
            self.layernorm.weight, self.layernorm.bias = frozen(p.ln_gamma[i]), frozen(p.ln_beta[i])


class _CspFfn(nn.Module):
    def __init__(self, p: CspParams, device):
        super().__init__()
        self.layers = nn.ModuleList([_CspLayer(p, i, device) for i in range(len(p.widths))])


class _CspSpaEnc(nn.Module):
    def __init__(self, p: CspParams, device):
        super().__init__()
        self.ffn = _CspFfn(p, device)
        self.frequency_num, self.min_radius, self.max_radius = p.frequency_num, p.min_radius, p.max_radius
        self.freq_init, self.freq_list = p.freq_init, p.freq_list
        self.spa_embed_dim, self.input_embed_dim = p.num_filts, p.input_dim


class _CspLocEnc(nn.Module):
    def __init__(self, p: CspParams, device):
        super().__init__()
        self.spa_enc = _CspSpaEnc(p, device)
        self.num_filts = p.num_filts
        if p.class_emb is not None:
            # the class head (models.py:131): bias-free, frozen, a mirror like the net's tensors
            self.class_emb = nn.Linear(p.num_filts, p.num_classes, bias=False, device="meta")
            self.class_emb.weight = nn.Parameter(torch.as_tensor(p.class_emb, dtype=torch.float32, device=device),
                                                 requires_grad=False)
            self.num_classes = p.num_classes


class CspLocationModel(nn.Module):
    """``model.loc_model`` of 'CSP' / 'CSP_INat' (range.py:143, 149: ``get_csp(path)``, a
    ``LocationImageEncoder``): a module whose call maps (B,2) (lon, lat) degrees - used as they are - to the
    (B, num_filts) float32 location embedding on the engine's GPU (``forward(coords, return_feats=True)``
    there), and whose parameters are the feed-forward net's, frozen, float32, on that GPU, under the
    reference's names (``loc_enc.spa_enc.ffn.layers.{i}.linear.weight`` ...).  As for SatCLIP they are a
    read-only MIRROR: the arithmetic runs in the engine (csp_kernel.h) on its own packed copy.  The user head
    and the image decoder of the checkpoint are not loaded.  The class head (``class_emb``, models.py:135-173)
    is loaded with ``load_model(..., class_head=True)`` only: then ``loc_enc.class_emb.weight`` joins the
    parameters, ``num_classes`` is set, and ``forward(coords, class_of_interest, return_feats=False)``,
    ``eval_single_class`` and ``class_sum`` run it in the engine (csp_head_kernel.h)."""

    def __init__(self, engine, p: CspParams):
        super().__init__()
        self.loc_enc = _CspLocEnc(p, engine.device)
        self.loc_emb_dim = p.num_filts
        self.num_classes = p.num_classes if p.class_emb is not None else 0
        self.spa_enc_type = p.spa_enc_type
        self._engine = [engine]
        self._params = [p]
        engine.set_csp(p.kind, p.freq_list, p.widths, p.weights, p.biases, p.ln_gamma, p.ln_beta,
                       CSP_ACTIVATIONS[p.activation], p.skip_connection, p.use_layn)
        if p.class_emb is not None:
            engine.set_csp_head(p.class_emb)
        self.eval()

    @property
    def csp_params(self) -> CspParams:
        """The ``CspParams`` of the installed network (the checkpoint's, or the last ``set_network``'s)."""
        return self._params[0]

    def set_network(self, p: CspParams) -> None:
        """Install a whole network - a trained one (range_amd.csp_fit) - in place of the loaded one: the encoder
        through the engine's ``set_csp`` and, when ``p.class_emb`` is set, its head through ``set_csp_head`` (without
        one the model has no head afterwards: a head belongs to the network it was fitted behind).  The mirror
        parameters, ``loc_emb_dim``, ``num_classes`` and ``spa_enc_type`` follow."""
        tensors = list(p.weights) + list(p.biases) + [a for a in list(p.ln_gamma) + list(p.ln_beta) if a is not None]
        if p.class_emb is not None:
            tensors.append(p.class_emb)
        if any(np.asarray(a).dtype != np.float32 or not np.isfinite(a).all() for a in tensors):
            raise ValueError("set_network: every tensor must be float32 and finite")
        eng = self._engine[0]
        eng.set_csp(p.kind, p.freq_list, p.widths, p.weights, p.biases, p.ln_gamma, p.ln_beta,
                    CSP_ACTIVATIONS[p.activation], p.skip_connection, p.use_layn)
        if p.class_emb is not None:
            eng.set_csp_head(p.class_emb)
        self.loc_enc = _CspLocEnc(p, eng.device)
        self.loc_emb_dim = p.num_filts
        self.num_classes = p.num_classes if p.class_emb is not None else 0
        self.spa_enc_type = p.spa_enc_type
        self._params = [p]

    def set_class_head(self, weight) -> None:
        """Install a class head - a fitted one (range_amd.head_fit) - behind the network: ``weight`` (num_classes,
        num_filts) float32, numpy or torch, finite.  It goes through the engine's ``set_csp_head`` like a checkpoint's,
        ``num_classes`` is set and ``loc_enc.class_emb.weight`` joins (or replaces) the mirror parameters, so that
        ``forward(return_feats=False)``, ``eval_single_class``, ``class_sum``, ``label_ranks``, ``GridPredictor`` and
        ``compute_acc_batch`` work on a model loaded without ``class_head=True``."""
        w = weight.detach().cpu().numpy() if torch.is_tensor(weight) else np.asarray(weight)
        if w.dtype != np.float32 or w.ndim != 2 or w.shape[1] != self.loc_emb_dim:
            raise ValueError(f"class head: float32 (num_classes, {self.loc_emb_dim}), got {w.dtype} {w.shape}")
        if not 1 <= w.shape[0] <= 32768:
            raise ValueError(f"class head: num_classes={w.shape[0]}: 1 .. 32768 are supported")
        if not np.isfinite(w).all():
            raise ValueError("class head: non-finite weights")
        w = np.ascontiguousarray(w)
        eng = self._engine[0]
        eng.set_csp_head(w)
        enc = self.loc_enc
        enc.class_emb = nn.Linear(self.loc_emb_dim, w.shape[0], bias=False, device="meta")
        enc.class_emb.weight = nn.Parameter(torch.as_tensor(w, dtype=torch.float32, device=eng.device), requires_grad=False)
        enc.num_classes = w.shape[0]
        self.num_classes = w.shape[0]

    def _need_head(self, what: str):
        if not self.num_classes:
            raise NotImplementedError(f"CSP: {what} needs the class head - load_model(..., class_head=True); without it "
                                      "only return_feats=True (the location embedding) is implemented")

    @staticmethod
    def _class_arg(class_of_interest):
        """-> (ids or None, scalar?): an int / 0-d tensor is one class -> (B,), a 1-D sequence / tensor -> (B, M)."""
        c = class_of_interest
        if c is None:
            return None, False
        if torch.is_tensor(c):
            if c.dim() == 0:
                return [int(c)], True
            return c, False
        a = np.asarray(c)
        if a.ndim == 0:
            return [int(a)], True
        return a, False

    @torch.no_grad()
    def forward(self, coords, class_of_interest=None, return_feats: bool = True):
        """``return_feats=True`` (the default here: the embedding is what ``model(coords)`` is made of): the (B,
        num_filts) embedding.  ``return_feats=False``: the reference's ``forward`` - (B, num_classes) float32
        probabilities, with ``class_of_interest`` an int / 0-d tensor (B,), a 1-D sequence or tensor of ids (B, M)."""
        if return_feats:
            return self.encode(_as_coords(coords, self._engine[0].device))
        self._need_head("return_feats=False")
        x = _as_coords(coords, self._engine[0].device)
        ids, scalar = self._class_arg(class_of_interest)
        out = self._engine[0].csp_predict(x, ids, _native.CSP_HEAD_PROBS)
        return out[:, 0] if scalar else out

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        """``x``: (B,2) float64 on the engine's GPU -> (B, num_filts) float32."""
        if x.shape[0] == 0:
            return torch.empty((0, self.loc_emb_dim), dtype=torch.float32, device=x.device)
        return self._engine[0].csp_encode(x)

    @torch.no_grad()
    def eval_single_class(self, feats: torch.Tensor, class_of_interest):
        """models.py:162-173: ``feats`` (B, num_filts) float32 on the GPU -> the raw logits, no sigmoid: (B,) for
        one class, (B, M) for a 1-D sequence or tensor of ids."""
        self._need_head("eval_single_class")
        ids, scalar = self._class_arg(class_of_interest)
        if ids is None:
            raise ValueError("eval_single_class needs a class_of_interest")
        out = self._engine[0].csp_head(feats.contiguous(), ids, _native.CSP_HEAD_LOGITS)
        return out[:, 0] if scalar else out

    @torch.no_grad()
    def class_sum(self, coords) -> torch.Tensor:
        """``self(coords, return_feats=False).sum(1)`` - (B,) float32 - without the (B, num_classes) matrix: the
        sum is formed in the kernel (float32, a fixed order)."""
        self._need_head("class_sum")
        return self._engine[0].csp_predict(_as_coords(coords, self._engine[0].device), None, _native.CSP_HEAD_SUM)

    #: label_ranks: bytes of image predictions on the GPU at a time
    img_chunk_bytes = 256 << 20

    @torch.no_grad()
    def label_ranks(self, coords, labels, img_preds=None):
        """What eval_helper.py's ``compute_acc_batch`` / ``get_label_rank`` make of ``self(coords, return_feats=False)``,
        without the (B, num_classes) matrix (csp_rank_kernel.h): ``coords`` (B,2) (lon, lat) degrees, ``labels`` (B,)
        integers, ``img_preds`` None or a numpy / torch array (B, num_classes), float32 or float64 (any other dtype is
        refused, not cast) -> (``ranks``, ``pred_classes``), numpy int64 (B,) each: the rank, from 1, of the label
        among the scores ``prior.double() * img_preds.double()`` (exact ties: the classes after the label count, as a
        stable argsort reversed ranks them) and the arg-max.  Rows the reference drops - a NaN / infinite location,
        a NaN score of the label - have rank 0 and class -1.  ValueError: a label outside ``[0, num_classes)``."""
        self._need_head("label_ranks")
        eng = self._engine[0]
        x = _as_coords(coords, eng.device)
        B, C = x.shape[0], self.num_classes
        lab = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
        if lab.shape != (B,) or lab.dtype.kind not in "iu":
            raise ValueError(f"labels: {B} integers, got {lab.dtype} {lab.shape}")
        if B and (lab.min() < 0 or lab.max() >= C):
            raise ValueError(f"labels outside 0 .. {C - 1}: min {lab.min()}, max {lab.max()}")
        lab_dev = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).to(eng.device)
        if img_preds is not None:
            if not torch.is_tensor(img_preds):
                img_preds = np.asarray(img_preds)
                if img_preds.dtype not in (np.float32, np.float64):
                    raise ValueError(f"img_preds must be float32 or float64, got {img_preds.dtype}")
                img_preds = torch.from_numpy(img_preds)
            if img_preds.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"img_preds must be float32 or float64, got {img_preds.dtype}")
            if tuple(img_preds.shape) != (B, C):
                raise ValueError(f"img_preds must be ({B}, {C}), got {tuple(img_preds.shape)}")
        ranks, pred = np.zeros(B, dtype=np.int64), np.full(B, -1, dtype=np.int64)
        step = B if img_preds is None else max(1, self.img_chunk_bytes // (C * img_preds.element_size()))
        for i in range(0, B, max(step, 1)):
            j = min(B, i + step)
            img = None if img_preds is None else img_preds[i:j].to(eng.device).contiguous()
            g, e, a = (t.cpu().numpy().astype(np.int64) for t in eng.csp_predict_rank(x[i:j], lab_dev[i:j], img))
            keep = g >= 0
            ranks[i:j][keep] = 1 + g[keep] + e[keep]
            pred[i:j][keep] = a[keep]
        return ranks, pred


class _EncoderBase(nn.Module):
    """What the one-GPU and the row-sharded encoder share: ``args``, ``engine``, ``loc_model``."""

    def _range_temperatures(self) -> int:
        """``args.temp`` / ``args.geo_temp`` (the reference's defaults unless ``load_model(temp=,
        geo_temp=)`` gave others) and the banner of RANGE / RANGE+; returns the kernel model id."""
        a = self.args
        check_temperatures(self.location_model_name, getattr(a, "temp", None), getattr(a, "geo_temp", None),
                           getattr(a, "pv_mode", None))
        a.temp, tau_geo, model_id, banner = range_model(self.location_model_name, getattr(a, "temp", None),
                                                        getattr(a, "geo_temp", None))
        if tau_geo:
            a.geo_temp = tau_geo
        print(banner)
        # what the engine runs at: its defaults are the reference's (range_set_temperatures)
        self._engine_temps = range_model(self.location_model_name)[:2]
        return model_id

    def _temperatures(self):
        """``args.temp`` / ``args.geo_temp`` as they are NOW - the reference reads them at every call
        (range.py:215, 234), like ``args.beta`` - validated -> (tau_sem, tau_geo); tau_geo = 0: RANGE."""
        a = self.args
        plus = self.location_model_name == "RANGE+"
        return check_temperatures(self.location_model_name, a.temp, a.geo_temp if plus else None,
                                  getattr(a, "pv_mode", None))

    def _sync_engine_temperatures(self):
        """The engine's forward at the current temperatures; a call into the library only when they changed."""
        temps = self._temperatures()
        if temps != self._engine_temps:
            self.engine.set_temperatures(*temps)
            self._engine_temps = temps
        return temps

    def _make_engine(self, enc, bank, row_offset: int = 0):
        a = self.args
        self._device = _device_of(a.device)
        return make_engine(enc, bank, self._device, row_offset, sh_eval=getattr(a, "sh_eval", None),
                           sh_source=getattr(a, "sh_source", None),
                           pv_mode=getattr(a, "pv_mode", None) if bank is not None else None)

    def _freeze(self):
        self.loc_model.eval()                                               # range.py:201-203
        for params in self.loc_model.parameters():
            params.requires_grad = False
        self.eval()

    def _coords(self, coords) -> torch.Tensor:
        return _as_coords(coords, self.engine.device)


class LocationEncoder(_EncoderBase):
    """RANGE / RANGE+ retrieval-augmented location encoder (reference: range/range.py:69)."""

    #: queries per engine call; bounds the per-call workspace (split slabs of chunk x 4 KB)
    chunk_size = 16384
    #: topk(): batches up to this size go through the HBM-streaming kernel in one call (bf16-key
    #: prefilter + float32 re-rank; one launch up to 256 queries: ~20 us for 16 queries on
    #: range_db_large, ~41 us for 64 (BENCH_r04.json roofline_scan) - faster than pass 1 + a selection
    #: over its kept logits at every size, tools/topk_total_time.py); larger batches in chunks of this size
    topk_stream_max = 16384

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.location_model_name = args.location_model_name
        if "RANGE" in self.location_model_name:                        # range.py:76
            bank, enc = _load(args, with_bank=True)
            self.location_feature_dim = 1024 + 256                     # :86
            self._model_id = self._range_temperatures()
            self.encoder_params = enc
            self.n_bank_rows = bank.n_rows
            self.engine = self._make_engine(enc, bank)
            self.loc_model = SatCLIPLocationModel(self.engine, enc, self.chunk_size)   # :83-84
        elif self.location_model_name == "SatCLIP":                     # range.py:117-122
            print("Using SatCLIP")
            _, enc = _load(args, with_bank=False)
            self.location_feature_dim = 256
            self._model_id = None
            self.encoder_params = enc
            self.engine = self._make_engine(enc, None)
            self.loc_model = SatCLIPLocationModel(self.engine, enc, self.chunk_size)   # :119-121
        elif self.location_model_name in _COORD_MODELS:                 # range.py:152-162, 170-173
            mode, banner = _COORD_MODELS[self.location_model_name]
            print(banner)
            self.location_feature_dim = _native.COORD_DIMS[mode]
            self._model_id = None
            self._coord_mode = mode
            self._device = _device_of(args.device)
            self.engine = _native.HipEngine(self._device)
            self.loc_model = _CoordLocationModel(self.engine, mode)
        elif posenc.is_posenc_name(self.location_model_name):           # range.py:164-168, 176-188
            # (an unknown s2vec kind: NotImplementedError here; the reference's get_sphere2vec returns
            # None for it and the failure comes at the first call)
            spec = posenc.spec(self.location_model_name)
            print("Using Theory" if self.location_model_name == "Theory" else "Using sphere2vec")
            # the TRUE row width: the reference leaves 0 (Theory, the sphere kinds) or nothing (grid)
            # here and never reads it; the batch driver sizes its staging buffers from it
            self.location_feature_dim = spec.width
            self._model_id = None
            self._device = _device_of(args.device)
            self.engine = _native.HipEngine(self._device)
            self.loc_model = PosencLocationModel(self.engine, self.location_model_name)
            self._posenc = spec
        elif self.location_model_name in _CSP_MODELS:                   # range.py:140-150
            print(_CSP_MODELS[self.location_model_name])
            csp = read_csp_checkpoint(args.pretrained_path, class_head=bool(getattr(args, "class_head", False)))
            self.location_feature_dim = csp.num_filts                   # (256 for the published checkpoints: :144, :150)
            self._model_id = None
            self.csp_params = csp
            self._device = _device_of(args.device)
            self.engine = _native.HipEngine(self._device)
            self.loc_model = CspLocationModel(self.engine, csp)
            self._csp = True
        else:
            # the reference dispatches more encoder families here (GeoCLIP, TaxaBind, SINR;
            # range.py:124-138, 190-197): third-party pretrained baselines that need their own
            # packages (geoclip, rshf) and download their weights, out of scope for this engine
            raise NotImplementedError(f"{self.location_model_name} not implemented")
        self._freeze()

    @torch.no_grad()
    def forward(self, coords, return_device: bool = False, return_topk: Optional[int] = None):
        """coords (B,2) float64 (lon,lat) deg -> (B,1280) float64 ``numpy.ndarray`` on the host
        (range.py:222/240).  ``return_device=True`` returns the device tensor instead (no D2H).

        ``return_topk=k`` (1..16; SURVEY.md 8(b) "Call" - the reference only hints at it,
        range.py:232): the call returns ``(embeddings, values (B,k) float32, indices (B,k) int64)``,
        the k bank rows most similar to each query (cosine, semantic keys; descending, ties to the
        lower row) as device tensors - ``model.topk(coords, k)``'s result bit for bit, from the SAME
        call: the queries are encoded once and the scan runs on the e-hat the forward left in the
        engine's workspace (``range_topk_last``).  A NaN / infinite coordinate gives a NaN row (as in
        the reference; rows are independent) and an undefined top-k for that row."""
        x = self._coords(coords)
        B = x.shape[0]
        if return_topk is not None:
            return self._forward_chunks(x, return_device, _topk_arg(return_topk, self._model_id is not None))
        if getattr(self, "_posenc", None) is not None:
            # Theory / s2vec_*: a device tensor of the coordinates' dtype (range.py:269-275)
            return self.loc_model.encode(x, self.loc_model.result_dtype(coords))
        if getattr(self, "_csp", False):
            # CSP / CSP_INat: a float32 device tensor whatever the coordinates' dtype (range.py:251-252)
            return self.loc_model.encode(x)
        if getattr(self, "_coord_mode", None) is not None:
            # Direct / Wrap return a device tensor, Cartesian_3D a host ndarray (its rad_to_cart
            # runs in numpy, range.py:265-268)
            d = self.location_feature_dim
            out = (self.engine.coord_features(x, self._coord_mode) if B else
                   torch.empty((0, d), dtype=torch.float64, device=x.device))
            if self._coord_mode == _native.COORD_CARTESIAN3D and not return_device:
                return out.cpu().numpy()
            return out
        if self._model_id is None:
            # plain SatCLIP: the un-normalised (B,256) float64 embedding, a device tensor like
            # the reference's (range.py:244-245)
            if B == 0:
                return torch.empty((0, 256), dtype=torch.float64, device=x.device)
            return torch.cat([self.engine.encode_raw(x[i:i + self.chunk_size])
                              for i in range(0, B, self.chunk_size)])
        return self._forward_chunks(x, return_device)

    def _forward_chunks(self, x: torch.Tensor, return_device: bool, k: Optional[int] = None):
        """The RANGE / RANGE+ forward in ``chunk_size`` slices, into a device tensor or
        (``return_device=False``, the reference's contract: range.py:240) a fresh host array filled slab by
        slab while the device->host copies of later slabs are in flight (range_forward_host); ``k``: with
        the top-k of every slice -> (out, values, rows).  (B == 0: nothing to launch; the reference returns
        an empty (0,1280) array as well)"""
        B = x.shape[0]
        beta = 1.0 if self._model_id == _native.MODEL_RANGE else float(self.args.beta)
        self._sync_engine_temperatures()
        if return_device:
            run, out = self.engine.forward, torch.empty((B, _native.OUT_DIM), dtype=torch.float64, device=x.device)
        else:
            run, out = self.engine.forward_host, POOL.take(B, _native.OUT_DIM)
        if k:
            tv = torch.empty((B, k), dtype=torch.float32, device=x.device)
            ti = torch.empty((B, k), dtype=torch.int64, device=x.device)
        for i in range(0, B, self.chunk_size):
            xc = x[i:i + self.chunk_size]
            n = xc.shape[0]
            run(xc, self._model_id, beta, out=out[i:i + n])
            if k:
                # (behind the forward on the same stream: the host result above is complete, the scan of
                # this chunk's e-hat runs while the caller - or the next chunk's encoder launch - goes on)
                tv[i:i + n], ti[i:i + n] = self.engine.topk_last(n, k)
        return (out, tv, ti) if k else out

    @torch.no_grad()
    def sweep(self, coords, betas=None, return_device: bool = False, *, temps=None, geo_temps=None):
        """RANGE+ embeddings of the same queries for several beta values (BASELINE config
        "beta sweep").  beta only enters the blend of range.py:238, so the semantic retrieval H
        and the geographic retrieval G are computed ONCE (two pass-2 launches instead of one per
        beta) and blended per beta with the reference's float32 rounding.
        Returns an array (len(betas), B, 1280) float64 (host ndarray, or device tensor).

        ``temps`` / ``geo_temps``: a TEMPERATURE sweep from one scan (``sweep_plan``).  H depends on
        ``temp`` alone and G on ``geo_temp`` alone, and the logits pass 1 keeps are un-scaled: per
        ``chunk_size`` slice the queries are encoded and scanned once, ONE ``stats_kept`` call gives the
        softmax statistics of every temperature from the kept logits, then one pass 2 per semantic and
        per geographic temperature and a blend + pack per grid point - T + G passes 2 for a T x G x nb
        grid.  RANGE+: (T, G, nb, B, 1280), a missing list being ``[args.temp]`` / ``[args.geo_temp]``
        and ``betas=None`` ``[args.beta]``.  RANGE (``temps`` only): (T, B, 1280), row i = ``model(coords)``
        at ``args.temp = temps[i]`` bit for bit.  H_i runs at the pair (temps[i], 0) and G_j at
        (12, geo_temps[j]) (beta = 0), so a head's bits do not depend on what else is in the lists:
        ``out[i, j, b]`` equals ``sweep(coords, betas)[b]`` at ``args.temp = temps[i]``,
        ``args.geo_temp = geo_temps[j]`` BIT FOR BIT whenever both lie on the same side of 43; when they
        straddle 43 that call runs both heads' statistics with a running maximum while here only the
        head above 43 does: equal within the usual bounds.  A slice whose logits were not kept (memory,
        RANGE_KEEP_LOGITS=0) takes ``scan_stats`` per pair and ``attend``: same bits, slower."""
        plan = sweep_plan(self.location_model_name, betas, temps, geo_temps, self.args.temp,
                          getattr(self.args, "geo_temp", None), getattr(self.args, "beta", None),
                          getattr(self.args, "pv_mode", None))
        if plan is not None:
            if self._model_id is None:
                raise ValueError("sweep() is defined for RANGE / RANGE+ only")
            return self._temperature_sweep(coords, plan, return_device)
        if self._model_id != _native.MODEL_RANGE_PLUS:
            raise ValueError("sweep() is defined for RANGE+ only")
        if betas is None:
            raise TypeError("sweep() needs betas (or temps= / geo_temps= for a temperature sweep)")
        betas = [float(b) for b in betas]
        tau_sem, tau_geo = self._temperatures()
        x = self._coords(coords)
        B = x.shape[0]
        out = torch.empty((len(betas), B, _native.OUT_DIM), dtype=torch.float64, device=x.device)
        eng = self.engine
        for i in range(0, B, self.chunk_size):
            e64, e32, xq = eng.encode(x[i:i + self.chunk_size])
            st = eng.scan_stats(e32, xq, tau_sem, tau_geo, keep_logits=True)
            kept = eng.kept_queries() == e32.shape[0]      # both passes 2 from the kept logits
            H, G = (attend_any(eng, kept, 0, e32, xq, tau_sem, tau_geo, b, st) for b in (1.0, 0.0))
            for j, b in enumerate(betas):
                out[j, i:i + e64.shape[0]] = eng.finalize(eng.blend(G, H, b), e64)
        return out if return_device else self._to_host(out)

    def _temperature_sweep(self, coords, plan: SweepPlan, return_device: bool):
        x = self._coords(coords)
        B = x.shape[0]
        out = torch.empty(plan.lead + (B, _native.OUT_DIM), dtype=torch.float64, device=x.device)
        eng = self.engine
        T = len(plan.temps)
        for i in range(0, B, self.chunk_size):
            e64, e32, xq = eng.encode(x[i:i + self.chunk_size])
            n = e64.shape[0]
            eng.scan_stats(e32, xq, *plan.scan_taus, keep_logits=True)
            kept = eng.kept_queries() == n
            if kept:
                stats = eng.stats_kept(0, xq, plan.pairs)          # ONE call for every pair of the grid
            else:
                stats = [eng.scan_stats(e32, xq, ts, tg) for ts, tg in plan.pairs]
            # one pass 2 per semantic temperature (beta = 1) and per geographic one (beta = 0)
            heads = [attend_any(eng, kept, 0, e32, xq, ts, tg, 1.0 if p < T else 0.0, stats[p])
                     for p, (ts, tg) in enumerate(plan.pairs)]
            for ti in range(T):
                if not plan.geo_temps:                              # RANGE: the semantic retrieval alone
                    out[ti, i:i + n] = eng.finalize(heads[ti], e64)
                    continue
                for gi in range(len(plan.geo_temps)):
                    for bi, b in enumerate(plan.betas):
                        out[ti, gi, bi, i:i + n] = eng.finalize(eng.blend(heads[T + gi], heads[ti], b), e64)
        return out if return_device else self._to_host(out)

    def _to_host(self, t: torch.Tensor) -> np.ndarray:
        """``.cpu()`` synchronises: a persistent launch of this call that gave up (NaN rows) is known
        now - report it instead of handing the rows out (range_hip.h: range_check_async_error)."""
        h = t.cpu().numpy()
        self.engine.check_async_error()
        return h

    @torch.no_grad()
    def topk(self, coords, k: int = 16):
        """Side channel: the k bank rows most similar (cosine, semantic keys) to each query,
        descending; returns (values (B,k) float32, indices (B,k) int64) device tensors."""
        x = self._coords(coords)
        if self._model_id is None:
            raise ValueError("topk() needs a bank (RANGE / RANGE+)")
        vals, idxs = [], []
        # the HBM-streaming kernel (every wave streams its own key tiles against 16 or 32 queries
        # per pass); the forward's own top-k (pass 1 keeps the logits anyway) is scan_stats(topk=k)
        for i in range(0, x.shape[0], self.topk_stream_max):
            _, e32, _ = self.engine.encode(x[i:i + self.topk_stream_max])
            tv, ti = self.engine.topk_stream(e32, k)
            vals.append(tv)
            idxs.append(ti)
        if len(vals) == 1:
            return vals[0], idxs[0]
        if not vals:
            return (torch.empty((0, k), dtype=torch.float32, device=x.device),
                    torch.empty((0, k), dtype=torch.int64, device=x.device))
        return torch.cat(vals), torch.cat(idxs)


class ShardedLocationEncoder(_EncoderBase):
    """RANGE / RANGE+ over a bank ROW-SHARDED across the ranks of a ``torch.distributed`` group (one
    process per GPU, backend "nccl" = RCCL over xGMI): ``load_model(..., shards=W)`` in every rank of
    a W-process job.  The reference has no distributed code; the call surface is its
    ``LocationEncoder``'s (range/range.py:69, :206-240), so the same script runs under
    ``torchrun --nproc-per-node W`` unchanged:

      ``model(coords)``              every rank passes the SAME (B,2) batch and gets the FULL
                                     (B,1280) float64 ``numpy.ndarray`` back (rank r embeds rows
                                     [r B/W, (r+1) B/W) against all shards, one all-gather of the
                                     results follows) - any B, also B < W;
      ``model(coords, local=True)``  data-parallel callers: ``coords`` are THIS rank's own queries
                                     (any count per rank, zero allowed), the result is their rows.

    Each rank loads and uploads only its rows of the bank (a ``.rbank`` file is memory-mapped, so a
    rank reads just its slice; an ``.npz`` is read whole by every rank and sliced)."""

    is_sharded = True

    def __init__(self, args, group=None):
        super().__init__()
        import torch.distributed as dist
        from .dist import ShardedRange, make_layout, shard_rows
        if not dist.is_available() or not dist.is_initialized():
            raise RuntimeError("load_model(..., shards=W) needs an initialised torch.distributed job "
                               "(torchrun --nproc-per-node W; range_amd.dist.init_from_env())")
        self.args = args
        self.location_model_name = args.location_model_name
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        want = getattr(args, "shards", None)
        if isinstance(want, int) and not isinstance(want, bool) and want != self.world:
            raise ValueError(f"shards={want} but the process group has {self.world} ranks")
        self._range_temperatures()
        bank, enc = _load(args, with_bank=True)
        self.location_feature_dim = 1024 + 256                           # :86
        self.encoder_params = enc
        self.n_bank_rows = bank.n_rows
        # 2-D layout (dist.make_layout): the bank row-sharded over `row_shards` ranks (default: all of
        # them), world / row_shards such groups each serving its own queries
        self.row_shards = int(getattr(args, "row_shards", None) or self.world)
        self.shard_group, shard_index, self.query_group = make_layout(self.row_shards, group)
        if self.n_bank_rows < self.row_shards:
            raise ValueError(f"bank of {self.n_bank_rows} rows cannot be sharded over {self.row_shards} ranks")
        self.row_range = shard_rows(bank.n_rows, self.row_shards, shard_index)
        self.engine = self._make_engine(enc, bank.rows(*self.row_range), row_offset=self.row_range[0])
        self.sharded = ShardedRange(self.engine, self.location_model_name, args.beta, group=self.shard_group,
                                    tau_sem=args.temp, tau_geo=getattr(args, "geo_temp", None))
        self.loc_model = SatCLIPLocationModel(self.engine, enc)          # range.py:83-84 (replicated on every rank)
        self._freeze()

    def _own_rows(self, B: int):
        return (B * self.rank) // self.world, (B * (self.rank + 1)) // self.world

    def _gather_rows(self, own: torch.Tensor, B: int, with_flags: bool = False):
        """Every rank's rows of a full-batch result -> the full result on every rank (one padded
        all-gather: the row counts differ by at most one).  ``with_flags`` (float64 rows): one more row
        travels with every rank's share, carrying its engine's give-up flag (range_async_error_flag:
        written on the device, in stream order behind the rank's kernels); returns (rows, (W,) flags)."""
        from .dist import start_collective
        W = self.world
        per = (B + W - 1) // W
        extra = 1 if with_flags else 0
        send = torch.zeros((per + extra,) + tuple(own.shape[1:]), dtype=own.dtype, device=own.device)
        send[:own.shape[0]] = own
        if with_flags:
            self.engine.async_error_flag(out=send[per].view(-1)[0:1])
        work, landed = start_collective("all_gather_into_tensor", send, self.group)
        work.wait()
        allr = landed()
        parts = []
        for r in range(W):
            n = (B * (r + 1)) // W - (B * r) // W
            parts.append(allr[r * (per + extra):r * (per + extra) + n])
        full = torch.cat(parts, dim=0)
        if not with_flags:
            return full
        return full, allr.view(W, per + 1, -1)[:, per, 0].clone()

    @torch.no_grad()
    def forward(self, coords, return_device: bool = False, local: bool = False, return_topk: Optional[int] = None):
        """``return_topk=k``: (embeddings, values (B,k) float32, GLOBAL bank rows (B,k) int64), the
        top-k from the same call (``LocationEncoder.forward``): the queries are encoded and gathered
        once, the per-shard candidates merge through ONE all-gather (``ShardedRange.forward``)."""
        x = self._coords(coords)
        k = None if return_topk is None else _topk_arg(return_topk)
        self.sharded.tau_sem, self.sharded.tau_geo = self._temperatures()
        if local:
            res = self.sharded.embed(x, topk=k)
            if not k:
                return res if return_device else self._to_host(res)
            return (res[0] if return_device else self._to_host(res[0])), res[1], res[2]
        B = x.shape[0]
        lo, hi = self._own_rows(B)
        res = self.sharded.embed(x[lo:hi], topk=k)
        own, tk = (res[0], res[1:]) if k else (res, ())
        full, flags = self._gather_rows(own, B, with_flags=True)
        tk = tuple(self._gather_rows(t, B).to(self.engine.device) for t in tk)
        emb = full.to(self.engine.device) if return_device else self._to_host(full, flags)   # range.py:240: a host ndarray
        return (emb, *tk) if k else emb

    @torch.no_grad()
    def sweep(self, coords, betas=None, return_device: bool = False, local: bool = False, *, temps=None, geo_temps=None):
        """(len(betas), B, 1280) float64 for several beta values (BASELINE config "beta sweep").
        ``temps`` / ``geo_temps``: the temperature sweep of ``LocationEncoder.sweep`` - (T, G, nb, B, 1280)
        for RANGE+, (T, B, 1280) for RANGE - from one scan per shard (``ShardedRange.sweep``)."""
        plan = sweep_plan(self.location_model_name, betas, temps, geo_temps, self.args.temp,
                          getattr(self.args, "geo_temp", None), getattr(self.args, "beta", None),
                          getattr(self.args, "pv_mode", None))
        if plan is None and self.location_model_name != "RANGE+":
            raise ValueError("sweep() is defined for RANGE+ only")
        if plan is None and betas is None:
            raise TypeError("sweep() needs betas (or temps= / geo_temps= for a temperature sweep)")
        x = self._coords(coords)
        self.sharded.tau_sem, self.sharded.tau_geo = self._temperatures()
        kw = {} if plan is None else dict(temps=temps, geo_temps=geo_temps)
        if local:
            out = self.sharded.embed_sweep(x, betas, **kw)
            return out if return_device else self._to_host(out)
        B = x.shape[0]
        lo, hi = self._own_rows(B)
        own = self.sharded.embed_sweep(x[lo:hi], betas, **kw)            # (..., b_own, 1280)
        lead = tuple(own.shape[:-2])
        flat = own.reshape((-1,) + tuple(own.shape[-2:]))
        full, flags = self._gather_rows(flat.permute(1, 0, 2).contiguous(), B, with_flags=True)
        full = full.permute(1, 0, 2).contiguous().reshape(lead + (B, own.shape[-1]))
        return full.to(self.engine.device) if return_device else self._to_host(full, flags)

    def _to_host(self, t: torch.Tensor, flags: Optional[torch.Tensor] = None) -> np.ndarray:
        """``.cpu()`` synchronises: a persistent launch of THIS rank that gave up is known now and is
        reported (range_hip.h: range_check_async_error).  ANOTHER rank's give-up arrives as its FLAG
        (``_gather_rows``: the rank's error word, written on the device behind its kernels, travels with
        its rows): every rank holds the same flags, so every rank refuses the result here - together,
        without a collective of its own.  The verdict comes from the word, never from the data: a NaN
        or infinite input coordinate gives a NaN row on every path - as in the reference, whose rows
        are independent - and is handed out like any other row."""
        h = t.cpu().numpy()
        bad = [] if flags is None else [int(r) for r in np.flatnonzero(flags.cpu().numpy() != 0.0)]
        self.engine.check_async_error()
        if bad:
            raise RuntimeError(f"sharded forward: a persistent launch of rank(s) {bad} of the group gave up (their rows of this "
                               "result are NaN; each reports it on its side and runs separate launches from now on): "
                               "re-issue the call")
        return h

    @torch.no_grad()
    def topk(self, coords, k: int = 16, local: bool = False):
        """Global top-k over all shards: (values (B,k) float32, global bank rows (B,k) int64)."""
        x = self._coords(coords)
        if local:
            return self.sharded.embed_topk(x, k)
        B = x.shape[0]
        lo, hi = self._own_rows(B)
        tv, ti = self.sharded.embed_topk(x[lo:hi], k)
        return (self._gather_rows(tv, B).to(self.engine.device), self._gather_rows(ti, B).to(self.engine.device))
