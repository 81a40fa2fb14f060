"""The WordPiece tokenizer of the host mirror (Vocab, tokenizer.ggml.model "bert": llama.cpp's
llm_tokenizer_wpm) through tests/cpp/t_bert.cpp, on a vocab-only model (no GPU): ids written out by
hand for the rules' edge cases, and agreement with a pure-Python restatement of the rules over
random strings.  Parity with llama.cpp itself is unpinned (it is not available offline)."""
import os
import struct
import subprocess
import unicodedata

import numpy as np

from blama_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "t_bert")

WORDS = ["pine", "##apple", "##s", "hello", "world", "cafe", "##\u0301", "un", "##able", "中", "[", "]", "5", "the", "##xy"]
CFG = synthetic.BertConfig("bert-tok", 300, 128, 1, 2, 128, 64)
VOCAB = synthetic.bert_vocab(CFG.n_vocab, words=WORDS)
ID = {t: i for i, t in enumerate(VOCAB["tokens"])}
PAD, UNK, CLS, SEP = 0, 1, 2, 3


def _binary():
    if not os.path.exists(BIN):   # host-only g++ build (no HIP compile); build() normally did it
        subprocess.run(["make", "-C", os.path.join(ROOT, "blama_amd", "host")], check=True, capture_output=True)
    return BIN


def tokenize(tmp_path, cases):
    """cases: (text, addSpecial, parseSpecial) -> the ids of each, by the C++ Vocab."""
    model, src, out = str(tmp_path / "m.gguf"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    synthetic.build_bert_gguf(CFG, header_only=True, vocab=VOCAB).tofile(model)
    with open(src, "wb") as f:
        for text, add, parse in cases:
            b = text.encode("utf-8")
            f.write(struct.pack("<BBI", int(add), int(parse), len(b)) + b)
    r = subprocess.run([_binary(), "--tok", f"--model={model}", f"--in={src}", f"--out={out}"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw = np.fromfile(out, np.int32)
    res, p = [], 0
    for _ in cases:
        n = int(raw[p])
        res.append([int(x) for x in raw[p + 1:p + 1 + n]])
        p += 1 + n
    assert p == raw.size
    return res


def ids(*pieces):
    return [p if isinstance(p, int) else ID["▁" + p[1:]] if p.startswith("_") else ID[p] for p in pieces]


def test_hand_written_cases(tmp_path):
    cases = [
        ("pineapples.", True, False, [CLS] + ids("_pine", "apple", "s", "_.") + [SEP]),
        # upper case and accented letters: NFD splits the accent off, then lowercase
        ("Hello CAF\u00c9 caf\u00e9", False, False, ids("_hello", "_cafe", "\u0301", "_cafe", "\u0301")),
        # an ASCII symbol without an entry is a word of its own: one [UNK] between its neighbours
        ("hello pine~q world", False, False, ids("_hello", "_pine") + [UNK] + ids("_q", "_world")),
        # "pine", "xy", "z", "z", "y" match, U+00FE has no entry: the whole word is one [UNK], nothing kept
        ("hello pinexyzzy\u00fe world", False, False, ids("_hello") + [UNK] + ids("_world")),
        # a CJK ideograph is a word of its own
        ("hello\u4e2dworld", False, False, ids("_hello", "_\u4e2d", "_world")),
        # leading, multiple and trailing spaces (and other white space)
        ("  hello \t\n  world\u00a0 ", False, False, ids("_hello", "_world")),
        ("", True, False, [CLS, SEP]),
        ("", False, False, []),
        ("hello world", False, False, ids("_hello", "_world")),
        # an ASCII symbol and punctuation split; control characters (Cc, Cf) vanish
        ("$5,hel\u200blo\x01!", False, False, ids("_$", "_5", "_,", "_hello", "_!")),
        # control-token texts: one token with parseSpecial, plain text without
        ("hello[SEP]world", False, True, ids("_hello") + [SEP] + ids("_world")),
        ("hello[SEP]world", False, False, ids("_hello", "_[", "_se", "p", "_]", "_world")),
        ("unable", True, True, [CLS] + ids("_un", "able") + [SEP]),
    ]
    got = tokenize(tmp_path, [(t, a, p) for t, a, p, _ in cases])
    for (text, add, parse, want), g in zip(cases, got):
        assert g == want, (text, add, parse, g, want, [VOCAB["tokens"][i] for i in g])


# ---- a pure-Python restatement of the rules ----
CJK = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
       (0x2B920, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))
INDEX = {t.encode("utf-8"): i for i, t in enumerate(VOCAB["tokens"])}
MAXLEN = max(len(b) for b in INDEX)


def wpm_ref(text, add):
    words = [""]
    for ch in unicodedata.normalize("NFD", text):
        c, cat = ord(ch), unicodedata.category(ch)
        if cat.startswith("Z") or 9 <= c <= 13 or c == 0x85:
            if words[-1]:
                words.append("")
            continue
        if c == 0 or c == 0xFFFD or cat in ("Cc", "Cf"):
            continue
        s = ch.lower()[0]
        if cat.startswith("P") or (c < 0x7F and cat.startswith("S")) or any(a <= c <= b for a, b in CJK):
            if words[-1]:
                words.append("")
            words[-1] = s
            words.append("")
        else:
            words[-1] += s
    out = [CLS] if add else []
    for w in words:
        if not w:
            continue
        b = ("▁" + w).encode("utf-8")
        i, piece = 0, []
        while i < len(b):
            j = min(len(b), i + MAXLEN + 1)
            while j > i and b[i:j] not in INDEX:
                j -= 1
            if j == i:
                piece = []
                break
            piece.append(INDEX[b[i:j]])
            i = j
        out += piece or [UNK]
    return out + ([SEP] if add else [])


ALPHABET = list("abcdehlnoprstuwxyz") * 3 + list("ABCHE") + [" "] * 8 + list("\t\n\u00a0\u3000") + list(".,!$[]-'+") + \
    list("\u00e9\u00c9\u0146\u0303\u0301\u0327\u00fe") + list("\u4e2d\u6587\u3400") + list("\u200b\x01\x7f\ufffd") + \
    list("57") + ["\uac00", "\ud55c", "\u1e69", "\u0130"]   # Hangul (arithmetic NFD), two marks on one base, a two-code-point lower()


def test_matches_python_restatement(tmp_path):
    rng = np.random.default_rng(7)
    texts = ["".join(ALPHABET[k] for k in rng.integers(0, len(ALPHABET), int(rng.integers(0, 40)))) for _ in range(200)]
    texts += ["pineapples.", "q\u0301\u0327x \u0301\u0327"]   # marks out of canonical order
    cases = [(t, bool(i % 2), False) for i, t in enumerate(texts)]
    got = tokenize(tmp_path, cases)
    n_unk = 0
    for (t, add, _), g in zip(cases, got):
        want = wpm_ref(t, add)
        assert g == want, (t, add, g, want)
        n_unk += want.count(UNK)
    assert 0 < n_unk < sum(len(g) for g in got) // 2   # the alphabet reaches both outcomes
