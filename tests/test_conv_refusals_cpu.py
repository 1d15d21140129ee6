"""The exact codes with which the conv and weight-gradient entries refuse bad arguments (no launch: runs without a GPU).

The five conv entries and the single-launch weight gradients share their host-side checks (csrc/conv3x3_mfma.hip:
conv_args_missing / conv_params / conv_tiles / conv_chain_ok; csrc/wgrad3x3_mfma.hip: wgrad_params), and every entry
puts checks of its own between them.  Which code comes back when two violations coincide is decided by that order and is
part of what the library accepts and returns; one case per shared check, per rule of the chain contract and per place
where the order shows is pinned here."""
import ctypes as C

import pytest

ARG, ALIGN, UNSUPPORTED = -1, -2, -4
INT_MAX = 2**31 - 1

_buf = (C.c_float * 8192)()
_base = C.addressof(_buf)
_base += (-_base) % 64
_names = ("x", "w", "bias", "y", "res", "mask", "in_scale", "in_shift", "out_scale", "gap", "gate_add", "gate_out", "dot", "dy",
          "dy_scale", "dy_shift", "dw", "dbias", "workspace")
PTR = {n: _base + 256 * (i + 1) for i, n in enumerate(_names)}  # distinct 16-byte aligned stand-ins, never dereferenced
_views = []


def _view(H, W, Cn, sW=None):
    sW = Cn if sW is None else sW
    v = (C.c_int64 * 6)(H * W * sW, W * sW, sW, 0, 64, 1 << 30)
    _views.append(v)
    return C.addressof(v)


def _conv(L, entry, **o):
    """One conv call at (B, H, W) = (1, 8, 8), 64 -> 64, x, w, bias and y set; `o` overrides; NAME_off=4 moves a pointer."""
    d = dict(B=1, H=8, W=8, cin=64, cout=64, bias_n=1, bias_q=64, alpha=1.0, relu=0, select=0, storage=3, mode=1, up=0, kreal=0,
             ca_tail=None, x=PTR["x"], w=PTR["w"], bias=PTR["bias"], y=PTR["y"])
    d["xview"] = d["yview"] = _view(8, 8, 64)
    for k, val in o.items():
        if k.endswith("_off"):
            d[k[:-4]] = PTR[k[:-4]] + val
        elif k in PTR and val is True:
            d[k] = PTR[k]
        else:
            d[k] = val
    g = d.get
    maps = (g("res"), g("mask"), g("in_scale"), g("in_shift"))
    tail = (g("gap"), g("gate_add"), g("gate_out"), g("dot"), d["B"], d["H"], d["W"])
    head = (g("x"), g("xview"), g("w"), g("bias"), d["bias_n"], d["bias_q"], g("y"), g("yview"))
    if entry == "geo":
        return L.sisr_conv3x3_c64_geo(g("x"), g("xview"), g("w"), g("bias"), g("y"), g("yview"), g("gap"), d["B"], d["H"], d["W"],
                                      d["cin"], d["cout"], d["mode"], d["up"], d["kreal"], None)
    if entry == "bf16s":
        return L.sisr_conv3x3_c64_bf16s(*head, *maps, d["alpha"], d["relu"], *tail, d["storage"], None)
    args = (*head, *maps, g("out_scale"), d["alpha"], d["relu"], *tail, d["cin"], d["cout"])
    if entry == "fp32":
        return L.sisr_conv3x3_c64(*args, d["ca_tail"], d["select"], None)
    return getattr(L, "sisr_conv3x3_c64_" + entry)(*args, d["select"], None)


GATE = dict(gate_add=True, gate_out=True, in_scale=True)
DOT = dict(dot=True, gap=True)
HUGE = dict(B=INT_MAX, H=5, W=33)  # 2 x 2 tiles per sample: more than 2^31 - 1 tiles
CONV_CASES = [
    # the shared steps, in every entry
    ("fp32", dict(x=None), ARG), ("bf16", dict(yview=None), ARG), ("x3", dict(w=None), ARG), ("bf16s", dict(y=None), ARG),
    ("geo", dict(xview=None), ARG), ("fp32", dict(B=0), ARG), ("bf16", dict(H=0), ARG), ("geo", dict(W=-1), ARG),
    ("fp32", dict(x_off=4), ALIGN), ("bf16", dict(w_off=4), ALIGN), ("x3", dict(in_scale_off=8), ALIGN),
    ("fp32", dict(in_scale=True, mask=True, in_shift_off=4), ALIGN), ("bf16s", dict(x_off=4), ALIGN), ("geo", dict(w_off=8), ALIGN),
    ("geo", dict(y_off=4), ALIGN), ("bf16s", dict(y_off=4), ALIGN),                      # y: these two entries only
    ("bf16s", dict(res_off=4), ALIGN), ("bf16s", dict(mask_off=4), ALIGN), ("bf16s", dict(gap=True, dot_off=4), ALIGN),
    ("bf16s", dict(GATE, gate_add_off=4), ALIGN), ("bf16s", dict(GATE, gate_out_off=4), ALIGN),
    ("fp32", dict(xview=_view(8, 8, 64, 66)), ALIGN), ("bf16", dict(xview=_view(8, 8, 64, 66)), ALIGN),
    ("x3", dict(xview=_view(8, 8, 64, 66)), ALIGN), ("geo", dict(xview=_view(8, 8, 64, 66)), ALIGN),
    ("bf16s", dict(dict.fromkeys(("xview", "yview"), _view(8, 8, 64, 68))), ALIGN),   # 2-byte elements: strides in eights
    ("fp32", HUGE, ARG), ("bf16", HUGE, ARG), ("x3", HUGE, ARG), ("bf16s", HUGE, ARG), ("geo", HUGE, ARG),
    ("fp32", dict(cin=60), UNSUPPORTED), ("bf16", dict(cout=0), UNSUPPORTED), ("x3", dict(cin=-64), UNSUPPORTED),
    ("geo", dict(cout=60), UNSUPPORTED),
    # the chain contract (fp32, bf16, x3: one predicate; a misaligned gate is "unsupported" there)
    ("fp32", dict(gate_add=True), UNSUPPORTED), ("bf16", dict(gate_out=True), UNSUPPORTED),
    ("x3", dict(gate_add=True, gate_out=True), UNSUPPORTED),                              # GATE needs in_scale
    ("fp32", dict(GATE, **DOT), UNSUPPORTED), ("bf16", dict(dot=True), UNSUPPORTED),      # GATE and DOT; DOT needs partial sums
    ("x3", dict(DOT, in_scale=True), UNSUPPORTED), ("fp32", dict(GATE, in_shift=True), UNSUPPORTED),
    ("bf16", dict(DOT, mask=True), UNSUPPORTED), ("x3", dict(GATE, out_scale=True), UNSUPPORTED),
    ("fp32", dict(DOT, cin=128, xview=_view(8, 8, 128)), UNSUPPORTED), ("bf16", dict(GATE, cout=128), UNSUPPORTED),
    ("fp32", dict(GATE, gate_add_off=4), UNSUPPORTED), ("x3", dict(GATE, gate_out_off=4), UNSUPPORTED),
    ("fp32", dict(DOT, yview=_view(8, 8, 64, 128)), UNSUPPORTED), ("bf16", dict(GATE, yview=_view(8, 8, 64, 128)), UNSUPPORTED),
    # ... and the bf16-storage entry's variant of it: asked of every call; mask / shift only beside a GATE
    ("bf16s", dict(yview=_view(8, 8, 64, 128)), UNSUPPORTED), ("bf16s", dict(gate_add=True), UNSUPPORTED),
    ("bf16s", dict(dot=True), UNSUPPORTED), ("bf16s", dict(GATE, mask=True), UNSUPPORTED), ("bf16s", dict(GATE, **DOT), UNSUPPORTED),
    # what each entry checks of its own
    ("fp32", dict(select=1), ARG), ("fp32", dict(select=5), ARG), ("fp32", dict(select=17), ARG), ("fp32", dict(select=-1), ARG),
    ("fp32", dict(select=8), UNSUPPORTED), ("fp32", dict(select=11, cin=128, cout=128), ARG),
    ("fp32", dict(relu=3), ARG), ("fp32", dict(relu=7), ARG), ("fp32", dict(relu=4), ARG), ("fp32", dict(relu=2, res=True), UNSUPPORTED),
    ("bf16", dict(select=2), ARG), ("x3", dict(select=1), ARG), ("bf16", dict(relu=2), UNSUPPORTED), ("x3", dict(relu=-1), UNSUPPORTED),
    ("bf16", dict(in_shift=True), UNSUPPORTED), ("x3", dict(gap=True, mask=True), UNSUPPORTED),
    ("bf16s", dict(storage=16), ARG), ("bf16s", dict(storage=-1), ARG), ("bf16s", dict(storage=2), UNSUPPORTED),
    ("bf16s", dict(relu=2), UNSUPPORTED), ("bf16s", dict(gap=True, res=True), UNSUPPORTED),
    ("geo", dict(mode=0), ARG), ("geo", dict(mode=2, up=1), UNSUPPORTED), ("geo", dict(kreal=-1), UNSUPPORTED), ("geo", dict(H=1), ARG),
    # two violations at once: the order of the checks
    ("fp32", dict(x=None, cin=60), ARG), ("fp32", dict(x_off=4, cin=60), UNSUPPORTED),    # presence, channels, alignment
    ("fp32", dict(x_off=4, relu=3), ALIGN), ("fp32", dict(x_off=4, select=1), ARG),       # select before, relu after
    ("fp32", dict(HUGE, relu=2, res=True), UNSUPPORTED),                                  # relu before the tile count ...
    ("fp32", dict(HUGE, gate_add=True), ARG), ("bf16", dict(HUGE, gate_add=True), UNSUPPORTED),  # ... the chain after it: fp32 only
    ("bf16", dict(HUGE, relu=2), UNSUPPORTED), ("x3", dict(HUGE, gap=True, mask=True), ARG),
    ("bf16", dict(x_off=4, relu=2), ALIGN), ("bf16s", dict(x_off=4, relu=2), UNSUPPORTED),  # bf16s: relu before alignment
    ("bf16", dict(x_off=4, gate_add=True), UNSUPPORTED), ("bf16", dict(x=None, gate_add=True), ARG),
    ("bf16s", dict(HUGE, storage=2), ARG), ("bf16s", dict(x=None, storage=16), ARG),
    ("geo", dict(mode=0, cin=60), UNSUPPORTED), ("geo", dict(mode=0, y_off=4), ARG), ("geo", dict(mode=2, up=1, H=1), UNSUPPORTED),
]


@pytest.mark.parametrize("k", range(len(CONV_CASES)))
def test_conv_entry_refusal_code(k):
    import sisr_amd
    entry, overrides, code = CONV_CASES[k]
    assert _conv(sisr_amd.hip.lib(), entry, **overrides) == code, (entry, overrides)


def _wgrad(L, entry, **o):
    d = dict(B=1, H=8, W=8, cin=64, cout=64, active=0, storage=1, up=0, co_real=64, ci_real=64, ws_delta=0, dy_scale=None,
             dy_shift=None, x=PTR["x"], dy=PTR["dy"], dw=PTR["dw"], dbias=PTR["dbias"], workspace=PTR["workspace"])
    d["xview"] = d["dyview"] = _view(8, 8, 64)
    for k, val in o.items():
        if k.endswith("_off"):
            d[k[:-4]] = PTR[k[:-4]] + val
        else:
            d[k] = val
    sizer = {"bf16": "bf16_", "bf16s": "bf16_", "x3": "x3_"}.get(entry, "")
    ws = max(0, getattr(L, f"sisr_wgrad3x3_c64_{sizer}workspace_bytes")(d["B"], d["H"], d["W"], d["cin"], d["cout"]) + d["ws_delta"])
    if entry == "geo":
        return L.sisr_wgrad3x3_c64_geo(d["x"], d["xview"], d["dy"], d["dyview"], d["dw"], d["co_real"], d["ci_real"], d["dbias"],
                                       d["workspace"], ws, d["B"], d["H"], d["W"], d["cin"], d["cout"], d["up"], d["active"], None)
    common = (d["x"], d["xview"], d["dy"], d["dyview"], d["dy_scale"], d["dy_shift"], 1.0, d["dw"], d["cin"] * 9, 9, 0, 1, 64, 1,
              64, d["dbias"], 1, 64, d["workspace"], ws, d["B"], d["H"], d["W"], d["cin"], d["cout"])
    if entry == "fp32":
        return L.sisr_wgrad3x3_c64(*common, d["active"], None)
    if entry == "bf16s":
        return L.sisr_wgrad3x3_c64_bf16s(*common, d["storage"], None)
    return getattr(L, "sisr_wgrad3x3_c64_" + entry)(*common, None)


WGRAD_CASES = [
    ("fp32", dict(x=None), ARG), ("geo", dict(dy=None), ARG), ("bf16", dict(dw=None), ARG), ("bf16s", dict(workspace=None), ARG),
    ("x3", dict(dyview=None), ARG), ("fp32", dict(B=0), ARG),
    ("fp32", dict(cin=60), UNSUPPORTED), ("bf16", dict(cout=0), UNSUPPORTED), ("x3", dict(cin=60), UNSUPPORTED),
    ("fp32", dict(ws_delta=-1), ARG), ("geo", dict(ws_delta=-1), ARG), ("bf16", dict(ws_delta=-1), ARG),
    ("bf16s", dict(ws_delta=-1), ARG), ("x3", dict(ws_delta=-1), ARG),
    ("fp32", dict(x_off=4), ALIGN), ("bf16", dict(dy_off=4), ALIGN), ("x3", dict(workspace_off=4), ALIGN),
    ("fp32", dict(dy_scale_off=4), ALIGN), ("bf16s", dict(dy_shift_off=8), ALIGN),
    ("fp32", dict(xview=_view(8, 8, 64, 66)), ALIGN), ("x3", dict(dyview=_view(8, 8, 64, 66)), ALIGN),
    ("bf16", dict(dyview=_view(8, 8, 64, 66)), ALIGN), ("bf16s", dict(xview=_view(8, 8, 64, 68)), ALIGN),  # bf16 maps: eights
    ("bf16s", dict(storage=3, dyview=_view(8, 8, 64, 68)), ALIGN),
    ("bf16s", dict(storage=0), ARG), ("bf16s", dict(storage=2), ARG), ("bf16s", dict(storage=4), ARG),
    ("fp32", dict(active=0x10), ARG), ("fp32", dict(active=0x1F), ARG),                   # bits beyond the four units
    ("fp32", dict(active=0x1), ARG),                                                      # a bias half nobody would sum
    ("fp32", dict(active=0x1, cin=1024, cout=1024), UNSUPPORTED),                         # more units than a mask holds
    ("geo", dict(co_real=65), ARG), ("geo", dict(ci_real=0), ARG), ("geo", dict(up=3), ARG), ("geo", dict(H=1), ARG),
    # two violations at once
    ("fp32", dict(x=None, cin=60), ARG), ("fp32", dict(cin=60, ws_delta=-1), UNSUPPORTED), ("bf16", dict(ws_delta=-1, x_off=4), ARG),
    ("x3", dict(x_off=4, xview=_view(8, 8, 64, 66), cout=60), UNSUPPORTED), ("bf16s", dict(storage=0, x=None), ARG),
    ("fp32", dict(active=0x10, x_off=4), ALIGN), ("geo", dict(co_real=65, x=None), ARG),
]


@pytest.mark.parametrize("k", range(len(WGRAD_CASES)))
def test_wgrad_entry_refusal_code(k):
    import sisr_amd
    entry, overrides, code = WGRAD_CASES[k]
    assert _wgrad(sisr_amd.hip.lib(), entry, **overrides) == code, (entry, overrides)
