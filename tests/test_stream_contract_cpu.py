"""The case table of the stream contract (tests/stream_cases.py) against include/relax_hip.h: every prototype with a relax_stream
parameter is a case or an exemption, never both, nothing else is listed, and every "waits" classification and every exemption quotes a
sentence of the comment that stands in front of that entry's prototype.  A new entry point cannot land without declaring its stream
behaviour.  No GPU."""
import os
import re

from tests import stream_cases as sc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "relax_hip.h")
PROTOTYPE = re.compile(r"^(?:int|int64_t|const char\*)\s+(relax_\w+)\s*\(([^;]*?)\)\s*;", re.M | re.S)


def _plain(text):
    """Comment decoration and line breaks out of the way: one line of words."""
    text = re.sub(r"/\*|\*/", " ", text)
    text = re.sub(r"^\s*\*\s?", " ", text, flags=re.M)
    return " ".join(text.split())


def header_entries():
    """-> ({C name: parameter list} of every prototype, {C name: the text between the prototype before it and itself, plain})"""
    src = open(HEADER).read()
    params, docs, at = {}, {}, 0
    for m in PROTOTYPE.finditer(src):
        params[m.group(1)] = " ".join(m.group(2).split())
        docs[m.group(1)] = _plain(src[at:m.start()])
        at = m.end()
    return params, docs


def stream_entries():
    return {name for name, p in header_entries()[0].items() if re.search(r"\brelax_stream\b", p)}


def test_the_parser_sees_the_whole_header():
    params, _ = header_entries()
    from relax_vqa_amd import _lib
    assert set(params) == set(_lib.PROTOTYPES), set(params) ^ set(_lib.PROTOTYPES)      # the ctypes table mirrors the header one to one
    assert "relax_flow_plan" not in stream_entries() and "relax_fragment_pairs" in stream_entries()


def test_every_stream_entry_is_a_case_or_exempt_and_nothing_else_is():
    want = stream_entries()
    assert len(want) == 68, len(want)       # today's count; a new entry point changes it here and declares itself in the table
    cased = {sc.entry_of(k) for k in sc.CASES}
    exempt = set(sc.EXEMPT)
    assert not cased & exempt, cased & exempt
    assert cased | exempt == want, (sorted(want - cased - exempt), sorted((cased | exempt) - want))
    for key in sc.CASES:
        assert key == sc.entry_of(key) or sc.entry_of(key) in sc.CASES, f"{key}: a variant without its entry's own record"
    assert not set(sc.COMPOSITES) & want


def test_every_waits_record_quotes_its_entrys_comment():
    _, docs = header_entries()
    for key, case in {**sc.CASES, **sc.COMPOSITES}.items():
        assert case.kind in ("enqueue", "waits"), key
        if case.kind == "waits":
            assert case.sentence and _plain(case.sentence) in docs[sc.entry_of(key)], f"{key}: {case.sentence!r} is not in the header's comment"
        else:
            assert case.sentence is None, key
    assert any(c.kind == "waits" for c in sc.CASES.values())


def test_every_exemption_has_a_reason_and_a_header_sentence():
    _, docs = header_entries()
    assert set(sc.EXEMPT) == set(sc.EXEMPT_BACKING)
    for name, reason in sc.EXEMPT.items():
        assert len(reason) > 20, name
        assert _plain(sc.EXEMPT_BACKING[name]) in docs[name], name


def test_records_are_well_formed():
    captured = set()
    for key, case in {**sc.CASES, **sc.COMPOSITES}.items():
        assert callable(case.make) and callable(case.call), key
        assert case.precisions is None or (set(case.precisions) <= set(sc.PRECISIONS) and case.precisions), key
        assert set(case.needs) <= {"rn50", "vit", "vgg16", "mlp", "trainer"}, key
        assert not (case.capture and case.kind == "waits"), f"{key}: a call that waits cannot be captured"
        if case.capture:
            captured.add(key)
    # the captures the contract is relied on for
    assert {"clip_vectors", "full_clip_vectors(flow=True)", "whole_residual_vectors", "relax_vgg16_features", "relax_vit_features_canvas",
            "relax_vit_intermediate_layers", "relax_resize_frames_ex", "relax_yuv_to_bgr_ex", "relax_fragment_pairs_ex", "relax_mlp_head",
            "relax_head_train_step_adam"} <= captured
    for key in ("clip_vectors", "full_clip_vectors(flow=True)"):
        assert sc.COMPOSITES[key].precisions == sc.PRECISIONS
    contracting = [k for k in sc.CASES if re.match(r"relax_(op_gemm|op_conv2d_nhwc|op_attention|op_attention_ex|resnet50|vgg16|vit_features|"
                                                   r"vit_intermediate)", k) and k != "relax_op_conv2d_nhwc_ex"]
    for key in contracting:
        assert sc.CASES[key].precisions == sc.PRECISIONS, key
