"""CPU: the registry of tests/devcontract.py covers every single-device bee2hip_*_dev entry include/bee2hip.h declares -- a new
_dev entry without a record (and so without its range, alignment, aliasing and capture checks in tests/test_gpu_dev_contract.py)
fails here -- and every record's smallest case can be made and has an oracle answer of the right shape."""
import numpy as np
import pytest

import devcontract as dc


def test_every_dev_entry_of_the_header_has_a_record():
    declared = dc.header_dev_symbols()
    assert len(declared) >= 27 and "bee2hip_bashF_batch_dev" in declared
    multi = {s for s in declared if s.endswith("_multi_dev")}
    assert set(dc.EXEMPT) == multi and all(len(why) > 20 for why in dc.EXEMPT.values())
    covered = {r.entry for r in dc.REGISTRY}
    assert covered | set(dc.EXEMPT) == declared, (sorted(declared - covered - set(dc.EXEMPT)), sorted(covered - declared))
    assert not covered & set(dc.EXEMPT)


def test_record_names_sizes_and_capture_marks():
    for r in dc.REGISTRY:
        assert r.sizes and len(set(map(dc.size_id, r.sizes))) == len(r.sizes), r.name
        assert (r.capture is None) != (r.why_not is None), r.name
    # the entries whose launch path cannot be captured, and only those
    assert {r.name for r in dc.REGISTRY if r.capture is None} == {"verify_keyed_128"}
    assert dc.resolve("cap", 256) == 256 * 2 * 1024 and dc.resolve((65, "cap+1"), 4) == (65, 8193)


@pytest.mark.parametrize("rec", dc.REGISTRY, ids=lambda r: r.name)
def test_smallest_case_of_every_record_has_inputs_and_an_oracle_answer(orc, rec):
    size = dc.resolve(rec.sizes[0], 256)
    a, b = rec.make(orc, size, 3), rec.make(orc, size, 4)
    assert a.args.keys() == b.args.keys() and all(np.array_equal(a.args[k], b.args[k]) for k in a.args), "host arguments depend on the seed"
    assert [(x.name, len(x.data), x.align, x.out) for x in a.bufs] == [(x.name, len(x.data), x.align, x.out) for x in b.bufs]
    assert all(x.align in (1, 4, 8, 16) for x in a.bufs) and any(x.out for x in a.bufs)
    lay = dc.Layout(a, 16)
    for x in a.bufs:
        s, n = lay.at[x.name]
        assert s % 256 == (16 if x.align == 16 else x.align) and s >= dc.GUARD and lay.total - s - n >= dc.GUARD
    img = lay.image(a, 99, orc)
    exp, mask = lay.expected(a, img, rec.expect(orc, a))
    assert mask.all() or rec.name.startswith("sde_")
    changed = np.nonzero(exp != img)[0]
    for pos in changed[[0, -1]] if changed.size else []:
        assert "guard" not in lay.where(int(pos))
