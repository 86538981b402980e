"""Every single change of a proof: `mutants(objects)` takes a proof's object list (pickle.loads(proof)) and yields (label, new_objects),
each a deep copy of the list with exactly ONE change.  Plain Python: nothing here imports the library; a field element is recognised by
its class name and rebuilt with its own class and field object.

A label is "index|atom|class": the object's index in the stream, the atom inside it that changed ("-" for the object as a whole,
"member 3", "depth 0", ...) and the class of the change.  Value changes, by the object's type:

    bytes (a digest: a root)         bit0, bit7last                                 bit 0 of byte 0 / bit 7 of the last byte flipped
    field element                    plus_one, plus_p, literal_p                    value + 1 mod p / value + p where below 2^128 (another
                                                                                    representative of the residue) / the value p itself
    list or tuple of field elements  the three above on the first, the middle and the last member (thin: the first and the last);
                                     swap_members (the first two, where they differ), drop_member (the middle one), repeat_member (the first)
    list of digests (a path)         bit0, bit7last at the first, the middle and the last depth (thin: the first and the last);
                                     drop_digest (the last), append_digest, swap_digests (the first adjacent two that differ)
    int (a nonce)                    nonce_plus_one, nonce_minus_one (at or above 0), nonce_2_64, nonce_as_element
    any object                       as_str

and per index the structural changes delete, and where objects follow: duplicate (in place), exchange (with the next object, where they are
not equal) and truncate (the stream ends behind this object).  Nothing is appended behind the last object: no verifier reads there.

Every index gets at least one mutant and an object of any other type is an error, both asserted here: a new kind of proof object cannot
pass unmutated."""
import pickle

BIT_CLASSES = ("bit0", "bit7last")
ELEMENT_CLASSES = ("plus_one", "plus_p", "literal_p")
SEQUENCE_CLASSES = ("swap_members", "drop_member", "repeat_member")
PATH_CLASSES = ("drop_digest", "append_digest", "swap_digests")
NONCE_CLASSES = ("nonce_plus_one", "nonce_minus_one", "nonce_2_64", "nonce_as_element")
VALUE_CLASSES = BIT_CLASSES + ELEMENT_CLASSES + SEQUENCE_CLASSES + PATH_CLASSES + NONCE_CLASSES + ("as_str",)
STRUCTURAL_CLASSES = ("delete", "duplicate", "exchange", "truncate")
# value changes after which every object has the type and the length it had and every field element is a residue below p
CANONICAL_CLASSES = BIT_CLASSES + ("plus_one", "swap_members", "swap_digests")


def label_index(label):
    return int(label.split("|")[0])


def label_atom(label):
    return label.split("|")[1]


def label_class(label):
    return label.split("|")[2]


def is_element(obj):
    return type(obj).__name__ == "FieldElement" and type(getattr(obj, "value", None)) is int and hasattr(obj, "field")


def kind_of(obj):
    """"digest", "element", "elements", "path" or "nonce"; TypeError for anything else"""
    if type(obj) is bytes:
        return "digest"
    if is_element(obj):
        return "element"
    if type(obj) in (list, tuple) and len(obj) > 0:
        if all(is_element(member) for member in obj):
            return "elements"
        if all(type(member) is bytes for member in obj):
            return "path"
    if type(obj) is int:
        return "nonce"
    raise TypeError("a proof object the enumerator does not know: %r" % (type(obj),))


def _flips(digest):
    yield "bit0", bytes([digest[0] ^ 1]) + digest[1:]
    yield "bit7last", digest[:-1] + bytes([digest[-1] ^ 0x80])


def _element_changes(element):
    p, make = element.field.p, type(element)
    yield "plus_one", make((element.value + 1) % p, element.field)
    if element.value + p < (1 << 128):
        yield "plus_p", make(element.value + p, element.field)
    yield "literal_p", make(p, element.field)


def _places(length, thin):
    places = [0, length - 1] if thin else [0, length // 2, length - 1]
    return sorted(set(places))


def _value_changes(obj, thin):
    """(atom, class, the changed object)"""
    kind = kind_of(obj)
    if kind == "digest":
        for name, changed in _flips(obj):
            yield "-", name, changed
    elif kind == "element":
        for name, changed in _element_changes(obj):
            yield "-", name, changed
    elif kind == "elements":
        make, members = type(obj), list(obj)
        for at in _places(len(members), thin):
            for name, changed in _element_changes(members[at]):
                yield "member %d" % at, name, make(members[:at] + [changed] + members[at + 1:])
        if len(members) > 1 and members[0].value != members[1].value:
            yield "members 0, 1", "swap_members", make([members[1], members[0]] + members[2:])
        middle = len(members) // 2
        yield "member %d" % middle, "drop_member", make(members[:middle] + members[middle + 1:])
        yield "member 0", "repeat_member", make(members[:1] + members)
    elif kind == "path":
        make, digests = type(obj), list(obj)
        for at in _places(len(digests), thin):
            for name, changed in _flips(digests[at]):
                yield "depth %d" % at, name, make(digests[:at] + [changed] + digests[at + 1:])
        yield "depth %d" % (len(digests) - 1), "drop_digest", make(digests[:-1])
        yield "depth %d" % len(digests), "append_digest", make(digests + [bytes(bytearray(digests[-1]))])
        for at in range(len(digests) - 1):
            if digests[at] != digests[at + 1]:
                yield "depths %d, %d" % (at, at + 1), "swap_digests", make(digests[:at] + [digests[at + 1], digests[at]] + digests[at + 2:])
                break
    else:
        yield "-", "nonce_plus_one", obj + 1
        if obj - 1 >= 0:
            yield "-", "nonce_minus_one", obj - 1
        yield "-", "nonce_2_64", 1 << 64
    yield "-", "as_str", "not a proof object"


def _same(left, right):
    """equal as proof objects (a field element compares by value with anything that has one: compare the pickles)"""
    return pickle.dumps(left) == pickle.dumps(right)


def _copy(objects):
    return pickle.loads(pickle.dumps(objects))


def mutants(objects, thin=False, element=None):
    """(label, new_objects) over every single change of `objects`.  thin: the first and the last member or depth of a sequence, not
    the first, the middle and the last.  element(value): how the nonce travels as a field element (nonce_as_element); without it the
    class and field object of the first field element found in the stream are used."""
    objects = list(objects)
    if element is None:
        found = None
        for obj in objects:
            for candidate in (obj if type(obj) in (list, tuple) else [obj]):
                if is_element(candidate):
                    found = candidate
                    break
            if found is not None:
                break

        def element(value, found=found):
            assert found is not None, "no field element in the stream to model the nonce's on"
            return type(found)(value, found.field)
    covered = set()
    for i, obj in enumerate(objects):
        for atom, name, changed in _value_changes(obj, thin):
            covered.add(i)
            yield "%d|%s|%s" % (i, atom, name), _copy(objects[:i] + [changed] + objects[i + 1:])
        if kind_of(obj) == "nonce":
            yield "%d|-|nonce_as_element" % i, _copy(objects[:i] + [element(obj)] + objects[i + 1:])
        yield "%d|-|delete" % i, _copy(objects[:i] + objects[i + 1:])
        if i + 1 < len(objects):
            # (a copy of the last object behind it would be an append, which no verifier reads; the two are copied apart: pickle would
            # write the second occurrence of one object as a reference)
            yield "%d|-|duplicate" % i, _copy(objects[:i + 1]) + _copy(objects[i:])
            if not _same(obj, objects[i + 1]):
                yield "%d|-|exchange" % i, _copy(objects[:i] + [objects[i + 1], obj] + objects[i + 2:])
            yield "%d|-|truncate" % i, _copy(objects[:i + 1])
    assert covered == set(range(len(objects))), "objects without a mutant: %s" % sorted(set(range(len(objects))) - covered)
