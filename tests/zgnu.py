"""The deflater extension restated in Python: a deflate tokenizer, the block rule of GNU
gzip's and Info-ZIP's deflater (ct_tally in their trees.c) on a token stream, and the raw walk's candidate list
with the GNU candidates in it.  Fixtures: tests/golden/gnu.json and gnu.bin (tests/golden/make_gnu.py).
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gnu.json")

LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)   # RFC 1951
CLORD = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LIT_BUFSIZE = 0x8000   # GNU's symbol buffer: a block holds at most LIT_BUFSIZE - 1 symbols


def fixtures():
    """gnu.json with each entry's body, and the archive's bytes, cut out of gnu.bin"""
    with open(GOLDEN) as f:
        g = json.load(f)
    with open(GOLDEN[:-5] + ".bin", "rb") as f:
        blob = f.read()
    for e in g["entries"]:
        e["body"] = blob[e["at"]:e["at"] + e["len"]]
    g["zip"]["bytes"] = blob[g["zip"]["at"]:g["zip"]["at"] + g["zip"]["len"]]
    return g


# ---- tokenizer ---------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, buf):
        self.b, self.pos, self.acc, self.n = buf, 0, 0, 0

    def get(self, k):
        while self.n < k:
            self.acc |= self.b[self.pos] << self.n
            self.pos += 1
            self.n += 8
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def align(self):
        self.acc, self.n = 0, 0


def _table(lens):
    """canonical Huffman code -> {(length, code): symbol}"""
    cnt = [0] * 16
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    t = {}
    for s, l in enumerate(lens):
        if l:
            t[(l, nxt[l])] = s
            nxt[l] += 1
    return t


def _sym(br, t):
    code, l = 0, 0
    while True:
        code = (code << 1) | br.get(1)
        l += 1
        s = t.get((l, code))
        if s is not None:
            return s
        assert l < 16, "bad Huffman code"


_FIXED_L = _table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_D = _table([5] * 30)


def tokenize(body):
    """A complete raw deflate stream -> (blocks, output, consumed).  A block is dict(btype, last, start, end,
    tokens): start / end are output positions; a token is (position, 0, byte) or (position, length, distance);
    a stored block's tokens are None (its bytes tell nothing of the parse behind them)."""
    br, out, blocks = _Bits(body), bytearray(), []
    while True:
        last, btype = br.get(1), br.get(2)
        blk = dict(btype=btype, last=last, start=len(out), tokens=[])
        if btype == 0:
            br.align()
            n = body[br.pos] | (body[br.pos + 1] << 8)
            assert n ^ 0xffff == body[br.pos + 2] | (body[br.pos + 3] << 8)
            out += body[br.pos + 4:br.pos + 4 + n]
            br.pos += 4 + n
            blk["tokens"] = None
        else:
            assert btype in (1, 2)
            if btype == 1:
                tl, td = _FIXED_L, _FIXED_D
            else:
                hlit, hdist, hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CLORD[i]] = br.get(3)
                tc, lens = _table(cl), []
                while len(lens) < hlit + hdist:
                    s = _sym(br, tc)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + br.get(2))
                    elif s == 17:
                        lens += [0] * (3 + br.get(3))
                    else:
                        lens += [0] * (11 + br.get(7))
                assert len(lens) == hlit + hdist
                tl, td = _table(lens[:hlit]), _table(lens[hlit:])
            toks = blk["tokens"]
            while True:
                s = _sym(br, tl)
                if s < 256:
                    toks.append((len(out), 0, s))
                    out.append(s)
                elif s == 256:
                    break
                else:
                    ln = LBASE[s - 257] + br.get(LEXT[s - 257])
                    d = _sym(br, td)
                    dist = DBASE[d] + br.get(DEXT[d])
                    assert dist <= len(out)
                    toks.append((len(out), ln, dist))
                    for _ in range(ln):
                        out.append(out[-dist])
        blk["end"] = len(out)
        blocks.append(blk)
        if last:
            break
    return blocks, bytes(out), br.pos


def no_repeated_trigram(data, a, b):
    """True when no three bytes starting in data[a:b] occur earlier in data (within 32 768 - 262 back) or twice:
    such a span parses to literals alone, whatever the level."""
    seen = {}
    for i in range(len(data) - 2):
        t = data[i:i + 3]
        if a <= i < b and t in seen and i - seen[t] <= 32768 - 262:
            return False
        seen[t] = i
    return True


def flat_tokens(blocks, data=None):
    """The stream's tokens in order.  A stored block stands for one literal per byte, which is its parse only when
    its span holds no repeated trigram: with `data` that is asserted."""
    out = []
    for b in blocks:
        if b["tokens"] is None:
            if data is not None:
                assert no_repeated_trigram(data, b["start"], b["end"]), "a stored block whose parse is not known"
            out += [(p, 0, data[p] if data is not None else -1) for p in range(b["start"], b["end"])]
        else:
            out += b["tokens"]
    return out


def symbol_counts(blocks):
    """symbols per block (a stored block: its bytes, see flat_tokens); the final block may be empty"""
    return [b["end"] - b["start"] if b["tokens"] is None else len(b["tokens"]) for b in blocks]


# ---- the block rule ------------------------------------------------------------------------------------
def dist_code(dist):
    for c in range(29, -1, -1):
        if dist >= DBASE[c]:
            return c
    raise ValueError(dist)


def gnu_blocks(tokens, level, trace=None):
    """ct_tally's flushes over a token stream (zlib's parse at this level, window 15, memLevel 8): the symbol count
    of every block, the final one included (it may be empty).  trace, a list, receives one
    (symbols of the block, last_dist, out, in) per evaluation of the heuristic."""
    counts = []
    last_lit = last_dist = 0
    dfreq = [0] * 30
    block_start = 0
    lazy = level >= 4   # the lazy parse tallies the symbol that starts at q one step late: strstart = q + 1
    for pos, ln, dist in tokens:
        last_lit += 1
        if ln:
            last_dist += 1
            dfreq[dist_code(dist)] += 1
        strstart = pos + 1 if lazy else pos
        flush = False
        if level > 2 and last_lit & 0xfff == 0:
            out = (last_lit * 8 + sum(dfreq[c] * (5 + DEXT[c]) for c in range(30))) >> 3
            inl = strstart - block_start
            if trace is not None:
                trace.append((last_lit, last_dist, out, inl))
            flush = last_dist < last_lit // 2 and out < inl // 2
        if last_lit == LIT_BUFSIZE - 1:
            flush = True
        if flush:
            counts.append(last_lit)
            last_lit = last_dist = 0
            dfreq = [0] * 30
            block_start = pos + (ln if ln else 1)
    counts.append(last_lit)
    return counts


# ---- the raw walk's list -------------------------------------------------------------------------------
MEMLEVELS = (8, 9, 7, 6, 5, 4, 3, 2, 1)
LEVELS = {0: (6, 9, 1, 5, 7, 8, 4, 3, 2, 0), 1: (1, 2, 3, 4, 5, 6, 7, 8, 9, 0), 2: (9, 8, 7, 6, 5, 4, 3, 2, 1, 0)}


def candidates(hint, gnu):
    """(level, window, memlevel) in the raw walk's order; memlevel 0 marks a GNU candidate."""
    out = []
    for m in MEMLEVELS:
        out += [(lv, 15, m) for lv in LEVELS[hint]]
        if m == 8 and gnu:
            out += [(lv, 15, 0) for lv in LEVELS[hint] if lv]
    return out


def packed(cand):
    lv, w, m = cand
    return (1 << 28) | (lv << 16) | (w << 8) | m
