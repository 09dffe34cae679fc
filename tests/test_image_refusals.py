"""The FIRST refusal of every entry point of the image, RGBA, YUV-frame and TTA-block families, pinned: tests/golden/image_call_refusals.json holds what
each answered -- return code and w2xc_last_error() text -- to calls with two independent things wrong at once (tests/golden/make_refusals.py wrote it and
builds the calls).  Which of the two a call names is the order of its argument checks; every recorded call is replayed and must answer the same, exactly.
No GPU: each of these calls is refused before a device is touched, and nothing is launched."""
import importlib.util
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def refusals(w2xc):
    spec = importlib.util.spec_from_file_location("make_refusals", os.path.join(GOLDEN, "make_refusals.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    models = gen.models(w2xc)
    return models, gen.cases(w2xc, models), gen.load()   # (the models outlive the calls)


def test_record_covers_the_families(refusals):
    _, calls, recorded = refusals
    names = {e.split("#")[0] for e in recorded}
    for family in ("w2xc_process_image_u8", "w2xc_process_image_rgb_u8", "w2xc_process_image_rgba_u8", "w2xc_process_frames_yuv_u8", "w2xc_tta_"):
        assert sum(n.startswith(family) for n in names) >= 4, family
    assert sum(len(v) for v in recorded.values()) >= 4000
    for entry, rows in recorded.items():
        for case, _, _ in rows:
            assert (entry, case) in calls, "a recorded case the generator no longer builds: %s %s" % (entry, case)


def test_first_refusal_is_the_recorded_one(w2xc, refusals):
    _, calls, recorded = refusals
    wrong = []
    for entry, rows in recorded.items():
        for case, rc, text in rows:
            got = calls[(entry, case)]()
            # (a call that got past its argument checks would run on the made-up addresses of the cases: none follows it)
            assert got[0] not in (w2xc.OK, w2xc.ERR_HIP), "%s [%s] is no longer refused: %r, recorded %r" % (entry, case, got, (rc, text))
            if got != (rc, text):
                wrong.append("%s [%s]: %r, recorded %r" % (entry, case, got, (rc, text)))
    assert not wrong, "%d of the recorded refusals changed:\n%s" % (len(wrong), "\n".join(wrong[:40]))
