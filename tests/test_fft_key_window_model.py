"""The key window of blind_rotate_fft_kernel (csrc/fft_kernels.hip, publish_mul_hook in csrc/fft_transform.h) as a
schedule: which key element sits in which window slot when a point of the transform meets it.

One iteration has two phases.  In the OWN phase the last forward stage (stage_lane<false, 1>) finishes the 16 points of
the wavefront's polynomial two at a time; every finished point p is multiplied by element p of the own key row and the
slot it used is refilled.  In the PARTNER phase, after the workgroup barrier, points c = 0..15 of the partner's
transform are multiplied by element c of the partner key row, and again the slot is refilled.  The model replays both
phases in program order with a window of W slots and the refill rule of the code, and checks that

  * every own-row point p and every partner-row point c is multiplied by element p (c) of the right row,
  * no slot is read before the request that fills it was issued (in program order),
  * no slot is overwritten while it holds an element that has not been used yet,
  * every element is requested exactly once and nothing is left in the window at the end.

The 4-point rule is the code's; the 8-point rule is the one it replaced, which ran bit-exact against the mirror for many
rounds: the model has to accept it as well, and has to reject rules that are wrong."""
import pytest

OWN, PAR = "own", "partner"


def last_stage_order(tau=1):
    """The (a, b) pairs in the order stage_lane<INV, TAU> hands them to its hook: G = 8 / TAU twiddle groups, for every
    even g the TAU butterflies of group g, then those of group g + 1 (the rotated twiddle)."""
    G = 8 // tau
    pairs = []
    for g in range(0, G, 2):
        for c in range(2 * g * tau, 2 * g * tau + tau):
            pairs.append((c, c + tau))
        if G > 1:
            for c in range(2 * (g + 1) * tau, 2 * (g + 1) * tau + tau):
                pairs.append((c, c + tau))
    return pairs


class Rule:
    """A window of `width` slots; own_refill(p) / par_refill(c) name the element requested into the slot just used."""

    def __init__(self, width, own_refill, par_refill, slot=None):
        self.width, self.own_refill, self.par_refill = width, own_refill, par_refill
        self.slot = slot or (lambda p: p & (width - 1))


RULE4 = Rule(4, lambda p: (OWN, p + 4) if p < 12 else (PAR, p - 12), lambda c: (PAR, c + 4) if c < 12 else None)
RULE8 = Rule(8, lambda p: (OWN, p + 8) if p < 8 else (PAR, p - 8), lambda c: (PAR, c + 8) if c < 8 else None)


class WindowError(AssertionError):
    pass


def replay(rule):
    """-> {(row, point): (step of the request, step of the use)}; raises WindowError on any violation."""
    slots = [None] * rule.width                  # (row, point, step of the request), None once used
    requested, log = set(), {}
    step = 0

    def request(slot, elem):
        if elem is None:
            return
        if not 0 <= elem[1] < 16:
            raise WindowError("request of %s element %d: not a key element" % elem)
        if slots[slot] is not None:
            raise WindowError("slot %d overwritten with %s %d while %s %d waits for its use" % ((slot,) + elem + slots[slot][:2]))
        if elem in requested:
            raise WindowError("%s element %d requested twice" % elem)
        requested.add(elem)
        slots[slot] = elem + (step,)

    def use(slot, elem):
        held = slots[slot]
        if held is None:
            raise WindowError("%s point %d reads slot %d before anything was requested into it" % (elem + (slot,)))
        if held[:2] != elem:
            raise WindowError("%s point %d meets %s element %d" % (elem + held[:2]))
        log[elem] = (held[2], step)
        slots[slot] = None

    for k in range(rule.width):                  # before the transform
        request(k, (OWN, k))
    for a, b in last_stage_order():              # publish_mul_hook: one(a); one(b)
        for p in (a, b):
            step += 1
            use(rule.slot(p), (OWN, p))
            request(rule.slot(p), rule.own_refill(p))
    for c in range(16):                          # after the barrier
        step += 1
        use(rule.slot(c), (PAR, c))
        request(rule.slot(c), rule.par_refill(c))
    if any(s is not None for s in slots):
        raise WindowError("left in the window: %r" % (slots,))
    if sorted(log) != sorted([(OWN, p) for p in range(16)] + [(PAR, c) for c in range(16)]):
        raise WindowError("not every point met a key element: %r" % sorted(log))
    return log


def test_the_last_stage_finishes_its_points_in_order():
    """The window relies on it: slot p & (W - 1) is free again exactly when point p + W needs requesting."""
    pairs = last_stage_order()
    assert [p for ab in pairs for p in ab] == list(range(16))
    assert all(b == a + 1 for a, b in pairs)


@pytest.mark.parametrize("rule", [RULE4, RULE8], ids=["window4", "window8"])
def test_every_point_meets_its_key_element(rule):
    log = replay(rule)
    # a request is always a whole window ahead of its use: W finished points of look-ahead, W - 1 .. W before the first
    for (row, p), (asked, used) in log.items():
        if row == OWN and p < rule.width:
            assert asked == 0
        else:
            assert used - asked == rule.width, (row, p, asked, used)


def test_partner_elements_are_requested_before_the_barrier_only_for_the_first_window():
    """Own steps are 1..16, partner steps 17..32: the partner row's first W elements are in flight across the barrier."""
    for rule in (RULE4, RULE8):
        log = replay(rule)
        early = sorted(c for (row, c), (asked, _) in log.items() if row == PAR and asked <= 16)
        assert early == list(range(rule.width))


@pytest.mark.parametrize("name,rule", [
    # the old refill distances in the new window: own point 8 would land on own point 4's successor
    ("old distances, 4 slots", Rule(4, RULE8.own_refill, RULE8.par_refill)),
    # the new distances with the old switch-over: own points 12..15 never requested
    ("switch-over at 8", Rule(4, lambda p: (OWN, p + 4) if p < 8 else (PAR, p - 8), RULE4.par_refill)),
    # partner refill one slot off
    ("partner slot off by one", Rule(4, RULE4.own_refill, lambda c: (PAR, c + 5) if c < 11 else None)),
    # partner refill past the end of the row
    ("partner refill not stopped", Rule(4, RULE4.own_refill, lambda c: (PAR, c + 4))),
    # the wrong row after the switch-over
    ("own row for ever", Rule(4, lambda p: (OWN, (p + 4) & 15), RULE4.par_refill)),
    # slot chosen by the old mask
    ("slot p & 7 in 4 slots", Rule(4, RULE4.own_refill, RULE4.par_refill, slot=lambda p: p & 7)),
])
def test_wrong_rules_are_rejected(name, rule):
    with pytest.raises((WindowError, IndexError)):
        replay(rule)
