"""The front end's band sums in the compiled kernel (group_bands in peaq_frontend.hip, peaq_group_sched.h), read from the
listing as tests/test_kernel_budgets.py reads the register budgets (hipcc cross-compiles for gfx950 without a GPU).

The wide band of a lane is fetched in pair slots, ds_read2_b64 with the slot's constant in the offset fields (slot j:
offset0 = 2 j, offset1 = 2 j + 1), group_batch_pairs slots to a batch.  What makes that cheaper than the loop it replaced
is that the reads of a batch are IN FLIGHT TOGETHER: the first straightforward version compiled to one
`s_waitcnt lgkmcnt(0)` behind every read, a round trip per pair.  So, for both instantiations and each of their two
call sites:
  * every slot 0 .. group_wide_pairs - 1 is there as one ds_read2_b64;
  * between the first and the last read of a batch no wait reaches a read of that batch.  The LDS queue returns in
    order, so `s_waitcnt lgkmcnt(N)` waits for all but the N youngest operations: with k LDS operations issued since
    the batch's first read (inclusive) a wait with N >= k is for OLDER data -- the tail of the batch before, which
    the compiler overlaps with these reads -- and is allowed; one with N < k would stall on the batch itself;
  * there is no branch from the first slot's read to the last one's: no loop, no divergence."""
import re

import pytest

from test_kernel_budgets import kernel_metadata

WIDE = {109: 12, 55: 25}       # group_wide_pairs
BATCH = {109: 4, 55: 5}        # group_batch_pairs
SITES = 2                      # 109: first band sums (one code path for both waves), noise spectrum; 55: the reference wave's two


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    d = tmp_path_factory.mktemp("fe_listing")
    kernel_metadata("peaq_frontend.hip", d)
    return (d / "peaq_frontend.hip.s").read_text().splitlines()


def kernel_body(lines, bands):
    start = next(i for i, l in enumerate(lines) if re.match(rf"^_Z\S*frontend_kernelILi{bands}E\S*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = []
    for l in lines[start + 1:end]:
        t = l.strip()
        if t and t[0] not in ";." and not t.endswith(":"):
            body.append(t)
    return body


def pair_slot(instr):
    """j of a pair-slot read (offsets 2 j and 2 j + 1), None for anything else"""
    m = re.match(r"ds_read2_b64 \S+ \S+(?: offset0:(\d+))?(?: offset1:(\d+))?$", instr)
    if not m:
        return None
    o0, o1 = int(m.group(1) or 0), int(m.group(2) or 0)
    return o0 // 2 if o0 % 2 == 0 and o1 == o0 + 1 else None


def wide_regions(body, bands):
    """per call site: {slot j: index of its read}, found backwards from the read of the last slot"""
    reads = [(i, pair_slot(t)) for i, t in enumerate(body) if t.startswith("ds_read2_b64")]
    regions = []
    for pos, (i, j) in enumerate(reads):
        if j != WIDE[bands] - 1:
            continue
        slots = {}
        for i2, j2 in reversed(reads[:pos + 1]):
            assert j2 is not None and j2 not in slots, (bands, "a read that is no pair slot inside the band sums", body[i2])
            slots[j2] = i2
            if len(slots) == WIDE[bands]:
                break
        assert sorted(slots) == list(range(WIDE[bands])), (bands, sorted(slots))
        regions.append(slots)
    return regions


@pytest.mark.parametrize("bands", [109, 55])
def test_reads_of_a_batch_are_in_flight_together(listing, bands):
    body = kernel_body(listing, bands)
    regions = wide_regions(body, bands)
    assert len(regions) == SITES, (bands, len(regions))
    for slots in regions:
        first_read, last_read = min(slots.values()), max(slots.values())
        for t in body[first_read:last_read + 1]:
            assert not re.match(r"s_cbranch|s_branch|s_setpc|s_call", t), (bands, "a branch inside the band sums", t)
        for j0 in range(0, WIDE[bands], BATCH[bands]):
            batch = [slots[j] for j in range(j0, min(j0 + BATCH[bands], WIDE[bands]))]
            first, last = min(batch), max(batch)
            waits = 0
            for i in range(first, last):
                m = re.match(r"s_waitcnt\b.*lgkmcnt\((\d+)\)", body[i])
                if not m:
                    continue
                issued = sum(1 for t in body[first:i] if t.startswith("ds_"))
                waits += 1
                assert int(m.group(1)) >= issued, (bands, j0, "a wait on the batch's own reads", body[i], issued)
            print(f"{bands} bands, slots {j0}..{j0 + len(batch) - 1}: {last - first + 1} instructions from first to last read, "
                  f"{waits} wait(s) for older data among them, none for these reads")

