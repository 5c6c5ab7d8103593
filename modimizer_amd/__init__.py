"""modimizer_amd — MI355X-native seqhash + modset hot path (libmodgpu.so) behind the reference's API.

This module is a thin ctypes binding over the C ABI declared in include/modgpu.h; all work happens
in the HIP library.  There is no CPU fallback: if the library or a HIP device is missing the batch
entry points raise.
"""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MODGPU_LIB") or os.path.join(_HERE, "libmodgpu.so")   # MODGPU_LIB: a variant build (tools/ablate_*.sh)
CSRC = os.path.join(_HERE, "csrc")

U64P = C.POINTER(C.c_uint64)
U32P = C.POINTER(C.c_uint32)

MG_POS_MASK = 0x7FFFFFFF
MG_FWD_BIT = 0x80000000


class Seqhash(C.Structure):            # include/modgpu.h (reference seqhash.h:15-23)
    _fields_ = [("seed", C.c_int), ("k", C.c_int), ("w", C.c_int), ("mask", C.c_uint64),
                ("shift1", C.c_int), ("shift2", C.c_int), ("factor1", C.c_uint64),
                ("factor2", C.c_uint64), ("patternRC", C.c_uint64 * 4)]


class SeqhashRCiterator(C.Structure):  # reference seqhash.h:25-34
    _fields_ = [("sh", C.POINTER(Seqhash)), ("s", C.c_void_p), ("sEnd", C.c_void_p),
                ("h", C.c_uint64), ("hRC", C.c_uint64), ("hashBuf", C.c_void_p), ("fBuf", C.c_void_p),
                ("base", C.c_int), ("iStart", C.c_int), ("iMin", C.c_int), ("isDone", C.c_bool)]


class Modset(C.Structure):             # reference modset.h:17-28
    _fields_ = [("hasher", C.POINTER(Seqhash)), ("tableBits", C.c_int), ("size", C.c_uint32),
                ("tableSize", C.c_uint64), ("tableMask", C.c_uint64), ("index", U32P),
                ("value", U64P), ("depth", C.POINTER(C.c_uint16)), ("info", C.POINTER(C.c_uint8)),
                ("max", C.c_uint32)]


class MgReference(C.Structure):       # include/modgpu.h (modmap.c:35-47)
    _fields_ = [("ms", C.POINTER(Modset)), ("size", C.c_uint32), ("max", C.c_uint32),
                ("index", U32P), ("offset", U32P), ("id", U32P), ("depth", U32P), ("rev", U32P), ("loc", U32P),
                ("nSeq", C.c_int), ("names", C.POINTER(C.c_char_p)), ("len", U32P)]


class MgReadset(C.Structure):         # include/modgpu.h (modasm.c:30-57,79-86)
    _fields_ = [("ms", C.POINTER(Modset)), ("nReads", C.c_int), ("capReads", C.c_int),
                ("len", C.POINTER(C.c_int)), ("nHit", C.POINTER(C.c_int)), ("nMiss", C.POINTER(C.c_int)),
                ("nCopy", C.POINTER(C.c_int * 4)), ("hitStart", U64P), ("hit", U32P), ("dx", C.POINTER(C.c_uint16)),
                ("totHit", C.c_uint64), ("capHit", C.c_uint64), ("invStart", U64P), ("invSpace", U32P),
                ("bad", C.POINTER(C.c_uint8)), ("contained", C.POINTER(C.c_int))]


class MgOverlaps(C.Structure):        # include/modgpu.h (modasm.c:291-298)
    _fields_ = [("n", C.c_uint32), ("start", U64P), ("iy", U32P), ("nHit", C.POINTER(C.c_uint16)), ("nBadOrder", C.POINTER(C.c_uint16)),
                ("nBadFlip", C.POINTER(C.c_uint16)), ("flags", C.POINTER(C.c_uint8))]


class MgModInfo(C.Structure):         # include/modgpu.h (ModInfo, modasm.c:61-77)
    _fields_ = [("flags", C.c_uint8), ("rDNApos", C.c_int), ("nGood", C.c_int), ("nMod2", C.c_int), ("nBadLD", C.c_int), ("nSplit", C.c_int), ("nSplitLD", C.c_int)]


class MgRepRef(C.Structure):          # include/modgpu.h (modrep.c:20-25)
    _fields_ = [("ms", C.POINTER(Modset)), ("len", C.c_int), ("pos", C.POINTER(C.c_int)), ("isF", C.POINTER(C.c_bool)), ("ownsMs", C.c_int)]


class MgRepResult(C.Structure):       # include/modgpu.h (modrep.c:170-268)
    _fields_ = [("nRead", C.c_int), ("nBad", C.c_int), ("nGood", C.c_int),
                ("n", C.POINTER(C.c_int)), ("seqF", C.POINTER(C.c_int)), ("seqR", C.POINTER(C.c_int)),
                ("bad", C.POINTER(C.c_bool)), ("isF", C.POINTER(C.c_bool)), ("max", C.c_uint32),
                ("modN", C.POINTER(C.c_int)), ("modNPre", C.POINTER(C.c_int)),
                ("goodI", C.POINTER(C.c_int)), ("goodLen", C.POINTER(C.c_int)), ("hitStart", U64P),
                ("hitK", C.POINTER(C.c_int)), ("hitX", C.POINTER(C.c_int)),
                ("nMod", C.c_int), ("nDup", C.c_int), ("tDup", C.c_int), ("minMax", C.c_int)]


class MgRep1Result(C.Structure):      # include/modgpu.h (modrep.c:272-489)
    _fields_ = [("nRead", C.c_int), ("nBad", C.c_int), ("nGood", C.c_int), ("max", C.c_uint32), ("nmod", (C.c_int * 4) * 5),
                ("readsBefore", C.c_int), ("readsAfter", C.c_int),
                ("modN", C.POINTER(C.c_int)), ("modNPre", C.POINTER(C.c_int)), ("modNPost", C.POINTER(C.c_int)),
                ("preStart", U64P), ("postStart", U64P),
                ("preK", C.POINTER(C.c_int)), ("preN", C.POINTER(C.c_int)), ("preX", C.POINTER(C.c_int)),
                ("postK", C.POINTER(C.c_int)), ("postN", C.POINTER(C.c_int)), ("postX", C.POINTER(C.c_int)),
                ("readI", C.POINTER(C.c_int)), ("hitStart", U64P), ("hitK", C.POINTER(C.c_int))]


class MgComposition(C.Structure):     # include/modgpu.h (composition.c:32-121)
    _fields_ = [("type", C.c_int), ("nSeq", C.c_uint64), ("totLen", C.c_uint64), ("lenMin", C.c_uint64), ("lenMax", C.c_uint64),
                ("base", C.c_uint64 * 256), ("qual", C.c_uint64 * 256), ("nBins", C.c_uint32), ("binCount", C.POINTER(C.c_int)), ("binSum", U64P)]


class MgSeqConvert(C.Structure):      # include/modgpu.h (seqconvert.c, seqhoco.c)
    _fields_ = [("inType", C.c_int), ("outType", C.c_int)] + [(n, C.c_uint64) for n in (
        "nSeq", "totSeqLen", "maxSeqLen", "totIdLen", "totDescLen", "maxIdLen", "maxDescLen", "nSeqIn", "totSeqLenIn")]


class MgGzMember(C.Structure):        # include/modgpu.h: a gzip member's deflate payload (offset and length without header and trailer), where its text goes, what its trailer states
    _fields_ = [("cOff", C.c_uint64), ("uOff", C.c_uint64), ("cLen", C.c_uint32), ("uLen", C.c_uint32), ("crc", C.c_uint32), ("pad", C.c_uint32)]


class MgGzBlock(C.Structure):         # include/modgpu.h: a block of text for the device's BGZF encoder: where it lies, its length (at most 65280)
    _fields_ = [("uOff", C.c_uint64), ("uLen", C.c_uint32), ("pad", C.c_uint32)]


class MgSeqBatch(C.Structure):        # include/modgpu.h
    _fields_ = [("bases", C.POINTER(C.c_int8)), ("offsets", C.POINTER(C.c_int64)), ("names", C.POINTER(C.c_char_p)),
                ("nSeq", C.c_int), ("total", C.c_int64), ("isFastq", C.c_int), ("basesCap", C.c_int64)]


# every symbol include/modgpu.h declares (tests check the library exports all of them)
EXPORTS = [
    "seqhashCreate", "seqhashWrite", "seqhashRead", "seqhashReport", "modRCiterator", "modRCnext",
    "minimizerRCiterator", "minimizerRCnext", "seqString", "mgSeqhashDestroy", "mgSeqhashRCiteratorDestroy",
    "modsetCreate", "modsetDestroy", "modsetWrite", "modsetRead", "modsetIndexFind", "modsetSummary",
    "modsetPack", "modsetDepthPrune", "modsetMerge",
    "mgLastError", "mgDeviceCount", "mgSetDevice", "mgVersion", "mgSourceHash", "mgDeviceAlloc", "mgDeviceFree",
    "mgMemcpyH2D", "mgMemcpyD2H", "mgMemsetD", "mgStreamSynchronize",
    "mgPackedWords", "mgPackHost", "mgPackDevice", "mgUnpackDevice", "mgUploadPack",
    "mgScanWorkBytes", "seqhashScanBatchDevice", "seqhashScanBatch", "seqhashMinimizerBatchDevice", "seqhashMinimizerBatch",
    "modsetAddBatchDevice", "modsetFindBatchDevice", "modsetSyncToHost", "mgXferThreadCount", "mgXferDiag", "mgCopyD2HBig", "mgCopyH2DBig", "mgModsetDeviceRelease",
    "mgModsetHostChanged", "modsetDepthHistogramDevice", "mgTableCheckLayout", "mgTableDiag", "mgScanDiag", "mgScanTailDiag", "mgScanBytesBelow", "mgValueWriterDiag", "mgAddReadsDevice", "mgQueryReadsDevice", "mgQueryReadsDeviceAsync", "mgQueryReadsDeviceWait",
    "mgAddSequenceBatch", "mgDepthHistogram", "mgSynthGenome", "mgSynthReads",
    "mgInsertReadsDevice", "mgAddSequences", "mgModsetWriteText", "mgReferenceCreate", "mgReferenceDestroy",
    "mgReferenceRead", "mgQueryProcess", "mgReferenceWrite", "mgGzipOpenWrite", "mgFzOpen", "mgGzipOpenRead", "mgReferenceLoad",
    "mgCommInitAll", "mgCommGetUniqueId", "mgCommInitRank", "mgCommRank", "mgCommSize", "mgCommDestroy", "mgHistogramAllReduce", "mgDepthAllReduce", "mgModsetMergeRankOrder",
    "mgReadsetCreate", "mgReadsetDestroy", "mgReadsetRead", "mgReadsetFileRead", "mgReadsetStats", "mgReadsetWrite", "mgReadsetLoad",
    "mgReadsetCleanMods", "mgReadsetCleanModsPath", "mgReadsetProperties", "mgReadsetPropertiesPath",
    "mgReadsetFindOverlaps", "mgOverlapsFree", "mgReadsetOverlapStats", "mgReadsetMarkBadReads", "mgReadsetMarkContained", "mgReadsetOverlapsPath", "mgReadsetOverlapsDiag",
    "mgReadsetRefFlagFile", "mgReadsetRefFlagHits", "mgReadsetResetBits", "mgReadsetTestMods", "mgReadsetModInfo", "mgReadsetReadFlags", "mgReadsetTestModsRun", "mgReadsetRdnaPath", "mgReadsetRdnaDiag", "mgReadsetRdnaGrid",
    "mgRepRefCreate", "mgRepRefFromArrays", "mgRepRefDestroy", "mgRepRunBegin", "mgRepRunAdd", "mgRepRunFinish", "mgRepResultFree", "mgRepAnalyze3File", "mgRepPath",
    "mgRep1ResultFree", "mgRepRunFinish1", "mgRepAnalyze1File", "mgRepAnalyze1Hits", "mgRepCount2", "mgRepAnalyze2File", "mgRep1Diag",
    "mgCompositionFile", "mgCompositionText", "mgCompositionFree", "mgCompositionDiag",
    "mgSeqConvertFile", "mgSeqConvertText", "mgSeqConvertDiag",
    "mgInflateMembersDevice", "mgInflateDiag", "mgInflateMemberHost", "mgBgzfInflateFile", "mgGzipInflateFile", "mgGunzipHost", "mgGunzipDiag", "mgGzipSrcDiag",
    "mgDeflateBlocksDevice", "mgDeflateBlockHost", "mgDeflateDiag", "mgBgzfDeflateFile", "mgSeqConvertFileBgzf",
    "mgSeqOpen", "mgSeqNextBatch", "mgSeqBatchFree", "mgSeqClose", "mgSeqReleaseBuffers", "mgReleaseBuffers", "mgTextParseFileDevice", "mgSeqOpenAt", "mgTextFileDiag", "mgAddSequenceFile", "mgReferenceFastaRead", "mgQueryFile",
    "mgReportDepths", "mgRefPaint", "mgRefPaintFile", "mgModsetWriteTextDevice", "mgModsetReadText", "mgModsetReadTextPath",
    "mgAddSequenceFile10x", "mgAddSequenceBatch10x", "mgTrim10xDevice", "mgAdd10xDiag",
    "mgModsetSetCopy", "mgModsetSetCopyM", "mgModsetSetCopyPath", "mgModsetSummaryDevice",
    "mgIterScanHost", "mgIterHostBelow", "mgReloadKnobs", "mgFormatF2", "mgModsetMergeArrays", "mgModsetMergeDeviceArrays", "mgModsetClear", "mgModsetDeviceSlots", "mgSetVerbose", "mgProfileEnable", "mgProfileOnly", "mgProfileReset", "mgProfileKernels", "mgProfileGet",
]


@contextlib.contextmanager
def knobs(**kv):
    """MODGPU_<NAME>=value (None: unset) for the duration of the block.  The library reads its environment knobs once
    (csrc/mg_knobs.c); mgReloadKnobs makes it read them again, on the way in and on the way out."""
    old = {}
    for k, v in kv.items():
        name = "MODGPU_" + k
        old[name] = os.environ.get(name)
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)
    lib().mgReloadKnobs()
    try:
        yield
    finally:
        for name, v in old.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
        lib().mgReloadKnobs()


def source_hash():
    """the hash csrc/Makefile bakes into the library (mg_version.c): sha256 over the `sha256sum` listing of every source, 16 hex digits"""
    import hashlib
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".c", ".h"))) + ["Makefile", "../../include/modgpu.h", "../../include/modgpu_compat.h"]
    inc = os.path.join(_HERE, "..", "include")
    path = lambda n: os.path.join(inc, os.path.basename(n)) if n.startswith("../") else os.path.join(CSRC, n)
    listing = "".join("%s  %s\n" % (hashlib.sha256(open(path(n), "rb").read()).hexdigest(), n) for n in names)
    return hashlib.sha256(listing.encode()).hexdigest()[:16]


def binary_hash(path=None):
    """the source hash a built libmodgpu.so carries, read out of the file (no dlopen); None if there is no such file or marker"""
    import re
    try:
        m = re.search(rb"MODGPU_SRC_HASH=([0-9a-f]{16})", open(path or LIB_PATH, "rb").read())
    except OSError:
        return None
    return m.group(1).decode() if m else None


def build(force=False):
    """Compile libmodgpu.so for gfx950 in-tree (hipcc cross-compiles without a GPU) whenever the binary is not the one these sources
    make: the hash baked into it differs from the tree's (a stale .so that rode along cannot be used), or it does not exist."""
    import fcntl
    if os.environ.get("MODGPU_LIB"):                    # a variant build under tools/: the caller's business
        return LIB_PATH
    def make_if_stale():
        if force or binary_hash() != source_hash():
            subprocess.check_call(["make", "-C", CSRC, "-j8", "-s"] + (["-B"] if force else []))
            if binary_hash() != source_hash():
                raise RuntimeError("libmodgpu.so does not carry the hash of its sources after make: %s != %s" % (binary_hash(), source_hash()))
    try:
        lk = open(os.path.join(CSRC, ".build.lock"), "w")     # tests start many processes: one make at a time
    except OSError:                                            # (a read-only tree: nothing to serialise, and nothing to build unless the binary is stale)
        make_if_stale()
        return LIB_PATH
    with lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        make_if_stale()
    return LIB_PATH


_lib = None


def lib():
    """Load libmodgpu.so, building it first if it is not the build of the sources in the tree. Raises if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if os.environ.get("MODGPU_NO_TORCH", "0") != "1":
        # torch bundles its own libamdhip64.so.7; load it first so both sides share ONE HIP runtime
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    build()
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    if not os.environ.get("MODGPU_LIB"):
        L.mgSourceHash.restype = C.c_char_p
        if L.mgSourceHash().decode() != source_hash():
            raise RuntimeError("the loaded libmodgpu.so was not built from the sources in this tree")
    vp, u64, u32, i32, i64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int64
    SH, MS, IT = C.POINTER(Seqhash), C.POINTER(Modset), C.POINTER(SeqhashRCiterator)

    def sig(name, res, *args):
        if os.environ.get("MODGPU_LIB") and not hasattr(L, name):      # a variant build of another round (A/B runs): what it lacks stays unbound
            return
        f = getattr(L, name); f.restype = res; f.argtypes = list(args)
    sig("seqhashCreate", SH, i32, i32, i32)
    sig("seqhashWrite", None, SH, vp); sig("seqhashRead", SH, vp); sig("seqhashReport", None, SH, vp)
    sig("modRCiterator", IT, SH, vp, i32)
    sig("modRCnext", C.c_bool, IT, U64P, C.POINTER(i32), C.POINTER(C.c_bool))
    sig("minimizerRCiterator", IT, SH, vp, i32)
    sig("mgIterScanHost", vp, SH, vp, i32); sig("mgIterHostBelow", i32, i32); sig("mgReloadKnobs", None)
    sig("mgFormatF2", i32, C.c_char_p, C.c_double)
    sig("minimizerRCnext", C.c_bool, IT, U64P, C.POINTER(i32), C.POINTER(C.c_bool))
    sig("seqString", C.c_char_p, u64, i32)
    sig("mgSeqhashDestroy", None, SH); sig("mgSeqhashRCiteratorDestroy", None, IT)
    sig("modsetCreate", MS, SH, i32, u32); sig("modsetDestroy", None, MS)
    sig("modsetWrite", None, MS, vp); sig("modsetRead", MS, vp)
    sig("modsetIndexFind", u32, MS, u64, i32); sig("modsetSummary", None, MS, vp)
    sig("modsetPack", C.c_bool, MS); sig("modsetDepthPrune", None, MS, i32, i32)
    sig("modsetMerge", C.c_bool, MS, MS)
    sig("mgLastError", C.c_char_p); sig("mgDeviceCount", i32); sig("mgSetDevice", i32, i32)
    sig("mgVersion", C.c_char_p)
    sig("mgSourceHash", C.c_char_p)
    sig("mgDeviceAlloc", i32, C.POINTER(vp), C.c_size_t); sig("mgDeviceFree", i32, vp)
    sig("mgMemcpyH2D", i32, vp, vp, C.c_size_t, vp); sig("mgMemcpyD2H", i32, vp, vp, C.c_size_t, vp)
    sig("mgMemsetD", i32, vp, i32, C.c_size_t, vp); sig("mgStreamSynchronize", i32, vp)
    sig("mgPackedWords", C.c_size_t, u64); sig("mgPackHost", None, vp, u64, vp)
    sig("mgUploadPack", i32, vp, u64, vp, vp); sig("mgPackDevice", i32, vp, u64, vp, vp); sig("mgUnpackDevice", i32, vp, u64, vp, vp)
    sig("mgScanWorkBytes", C.c_size_t, u64, u32, u64)
    sig("seqhashScanBatchDevice", i32, SH, vp, u64, vp, u32, vp, vp, vp, u64, vp, vp, vp)
    sig("seqhashScanBatch", i64, SH, vp, vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp))
    sig("seqhashMinimizerBatchDevice", i32, SH, vp, u64, vp, u32, vp, vp, vp, u64, U64P, vp)
    sig("seqhashMinimizerBatch", i64, SH, vp, vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp))
    sig("modsetAddBatchDevice", i32, MS, vp, u64, vp, i32, vp)
    sig("modsetFindBatchDevice", i32, MS, vp, u64, vp, vp)
    sig("modsetSyncToHost", i32, MS, i32); sig("mgXferThreadCount", i32); sig("mgXferDiag", None, U64P); sig("mgCopyD2HBig", i32, vp, vp, C.c_size_t); sig("mgCopyH2DBig", i32, vp, vp, C.c_size_t); sig("mgModsetDeviceRelease", i32, MS)
    sig("mgModsetHostChanged", None, MS)
    sig("modsetDepthHistogramDevice", i32, MS, vp, vp); sig("mgTableCheckLayout", i32, MS, U64P); sig("mgTableDiag", i32, MS, U64P); sig("mgScanDiag", i32, U64P); sig("mgScanTailDiag", i32, U64P); sig("mgScanBytesBelow", u32, u32, u32); sig("mgValueWriterDiag", i32, U64P)
    sig("mgAddReadsDevice", i32, MS, vp, u64, vp, u32, U64P, vp)
    sig("mgQueryReadsDevice", i32, MS, vp, u64, vp, u32, vp, vp, vp, u64, U64P, vp)
    sig("mgQueryReadsDeviceAsync", i32, MS, vp, u64, vp, u32, vp, vp, vp, u64, C.POINTER(vp), vp); sig("mgQueryReadsDeviceWait", i32, vp, U64P, vp)
    sig("mgAddSequenceBatch", i64, MS, vp, vp, i32); sig("mgDepthHistogram", None, MS, vp)
    sig("mgSynthGenome", i32, vp, u64, u64, vp)
    sig("mgSynthReads", i32, vp, u64, vp, vp, vp, u32, u64, C.c_double, u64, vp, vp)
    sig("mgInsertReadsDevice", i32, MS, vp, u64, vp, u32, vp, vp, vp, u64, U64P, vp)
    sig("mgAddSequences", i32, MS, vp, vp, i32, vp); sig("mgModsetWriteText", None, MS, vp)
    sig("mgReferenceCreate", vp, MS, u32); sig("mgReferenceDestroy", None, vp)
    sig("mgReferenceRead", i32, vp, vp, vp, i32, C.POINTER(C.c_char_p), C.c_bool, vp)
    sig("mgQueryProcess", i32, vp, vp, vp, i32, C.POINTER(C.c_char_p), vp)
    RS = C.POINTER(MgReadset)
    sig("mgReadsetCreate", RS, MS); sig("mgReadsetDestroy", None, RS)
    sig("mgReadsetRead", i32, RS, vp, vp, i32); sig("mgReadsetFileRead", i32, RS, C.c_char_p)
    sig("mgReadsetStats", None, RS, vp); sig("mgReadsetWrite", None, RS, C.c_char_p); sig("mgReadsetLoad", RS, C.c_char_p)
    sig("mgReadsetCleanMods", i32, RS, vp); sig("mgReadsetCleanModsPath", i32); sig("mgReadsetProperties", i32, RS, vp); sig("mgReadsetPropertiesPath", i32)
    sig("mgReadsetFindOverlaps", i32, RS, vp, C.c_uint32, i32, vp, C.POINTER(MgOverlaps)); sig("mgOverlapsFree", None, C.POINTER(MgOverlaps))
    sig("mgReadsetOverlapStats", i32, RS, C.c_uint32, vp); sig("mgReadsetMarkBadReads", i32, RS, vp); sig("mgReadsetMarkContained", i32, RS, vp)
    sig("mgReadsetOverlapsPath", i32); sig("mgReadsetOverlapsDiag", None, vp)
    sig("mgReadsetRefFlagFile", i32, RS, C.c_char_p, vp); sig("mgReadsetRefFlagHits", i32, RS, vp, vp, u64, vp); sig("mgReadsetResetBits", i32, RS, i32, vp)
    sig("mgReadsetTestMods", i32, RS, i32, i32, vp, vp, vp); sig("mgReadsetModInfo", C.POINTER(MgModInfo), RS); sig("mgReadsetReadFlags", C.POINTER(C.c_uint8), RS)
    sig("mgReadsetTestModsRun", i32, RS); sig("mgReadsetRdnaPath", i32); sig("mgReadsetRdnaDiag", None, vp); sig("mgReadsetRdnaGrid", None, vp)
    RR, RES = C.POINTER(MgRepRef), C.POINTER(MgRepResult)
    sig("mgRepRefCreate", RR, C.c_char_p, C.c_char_p, vp); sig("mgRepRefFromArrays", RR, MS, vp, i64, vp); sig("mgRepRefDestroy", None, RR)
    sig("mgRepRunBegin", vp, RR, MS); sig("mgRepRunAdd", i32, vp, vp, vp, i32, vp); sig("mgRepRunFinish", i32, vp, vp, RES); sig("mgRepResultFree", None, RES)
    sig("mgRepAnalyze3File", i32, RR, C.c_char_p, C.c_char_p, vp, vp, RES); sig("mgRepPath", i32)
    RES1 = C.POINTER(MgRep1Result)
    sig("mgRep1ResultFree", None, RES1); sig("mgRepRunFinish1", i32, vp, vp, vp, RES1); sig("mgRepAnalyze1File", i32, RR, C.c_char_p, C.c_char_p, vp, vp, RES1)
    sig("mgRepAnalyze1Hits", i32, C.c_uint32, i32, i32, vp, vp, vp, vp, vp, vp, RES1); sig("mgRepCount2", i32, RR, vp, vp, i32, vp)
    sig("mgRepAnalyze2File", i32, RR, C.c_char_p, C.c_char_p, vp, vp); sig("mgRep1Diag", None, vp)
    COMP = C.POINTER(MgComposition)
    sig("mgCompositionFile", i32, C.c_char_p, i32, vp, vp, COMP); sig("mgCompositionText", i32, vp, u64, i32, vp, vp, COMP)
    sig("mgCompositionFree", None, COMP); sig("mgCompositionDiag", None, vp)
    CONV = C.POINTER(MgSeqConvert)
    sig("mgSeqConvertFile", i32, C.c_char_p, C.c_char_p, i32, vp, CONV); sig("mgSeqConvertText", i32, vp, u64, i32, vp, vp, CONV); sig("mgSeqConvertDiag", None, vp)
    sig("mgInflateMembersDevice", i32, vp, u64, C.POINTER(MgGzMember), u32, vp, u64, vp, C.POINTER(u32), vp); sig("mgInflateDiag", None, vp)
    sig("mgInflateMemberHost", i32, vp, u32, vp, u32, u32, C.POINTER(u32), vp); sig("mgBgzfInflateFile", i32, C.c_char_p, C.c_char_p, vp)
    sig("mgGzipInflateFile", i32, C.c_char_p, C.c_char_p, vp); sig("mgGunzipDiag", None, vp); sig("mgGzipSrcDiag", None, vp)
    sig("mgGunzipHost", i32, vp, u64, u32, u32, u32, vp, u64, C.POINTER(u64), C.POINTER(u32), vp)
    sig("mgDeflateBlocksDevice", i32, vp, u64, C.POINTER(MgGzBlock), u32, vp, u64, C.POINTER(u64), vp); sig("mgDeflateDiag", None, vp)
    sig("mgDeflateBlockHost", i32, vp, u32, vp, C.POINTER(u32), vp); sig("mgBgzfDeflateFile", i32, C.c_char_p, C.c_char_p, vp)
    sig("mgSeqConvertFileBgzf", i32, C.c_char_p, C.c_char_p, i32, vp, CONV)
    sig("mgSeqOpen", vp, C.c_char_p); sig("mgSeqNextBatch", i32, vp, C.c_int64, C.POINTER(MgSeqBatch))
    sig("mgSeqBatchFree", None, C.POINTER(MgSeqBatch)); sig("mgSeqClose", None, vp); sig("mgSeqReleaseBuffers", None); sig("mgReleaseBuffers", None)
    sig("mgTextParseFileDevice", i32, C.c_char_p, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64))
    sig("mgSeqOpenAt", vp, C.c_char_p, u64, u64, u64); sig("mgTextFileDiag", None, vp)
    sig("mgAddSequenceFile", i32, MS, C.c_char_p, vp); sig("mgReferenceFastaRead", i32, vp, C.c_char_p, C.c_bool, vp)
    sig("mgQueryFile", i32, vp, C.c_char_p, vp)
    sig("mgReportDepths", i32, MS, C.POINTER(MS), i32, vp)
    sig("mgRefPaint", i32, MS, vp, vp, i32, C.POINTER(C.c_char_p), vp); sig("mgRefPaintFile", i32, MS, C.c_char_p, vp)
    sig("mgModsetWriteTextDevice", i32, MS, vp); sig("mgModsetReadText", MS, C.c_char_p); sig("mgModsetReadTextPath", i32)
    sig("mgAddSequenceFile10x", i32, MS, C.c_char_p, vp); sig("mgAddSequenceBatch10x", i64, MS, vp, vp, i32, u64)
    sig("mgTrim10xDevice", i32, vp, u64, vp, u32, u64, vp, vp, U64P, vp); sig("mgAdd10xDiag", None, U64P)
    sig("mgModsetSetCopy", i32, MS, i32, i32, i32); sig("mgModsetSetCopyM", i32, MS, i32); sig("mgModsetSetCopyPath", i32)
    sig("mgModsetSummaryDevice", i32, MS, vp)
    sig("mgReferenceWrite", None, vp, C.c_char_p); sig("mgGzipOpenWrite", vp, C.c_char_p); sig("mgGzipOpenRead", vp, C.c_char_p); sig("mgFzOpen", vp, C.c_char_p, C.c_char_p);
    sig("mgCommInitAll", i32, C.POINTER(vp), i32, C.POINTER(i32)); sig("mgCommGetUniqueId", i32, vp); sig("mgCommInitRank", i32, C.POINTER(vp), i32, i32, vp, i32)
    sig("mgCommRank", i32, vp); sig("mgCommSize", i32, vp); sig("mgCommDestroy", None, vp)
    sig("mgHistogramAllReduce", i32, MS, vp, vp); sig("mgDepthAllReduce", i32, MS, vp); sig("mgModsetMergeRankOrder", i32, MS, vp, i32)
    sig("mgReferenceLoad", C.POINTER(MgReference), C.c_char_p)
    sig("mgModsetMergeArrays", C.c_bool, MS, vp, vp, vp, u32)
    sig("mgModsetMergeDeviceArrays", C.c_bool, MS, vp, vp, vp, u32)
    sig("mgModsetClear", i32, MS, vp); sig("mgModsetDeviceSlots", u64, MS); sig("mgSetVerbose", None, i32)
    sig("mgProfileEnable", None, i32); sig("mgProfileOnly", None, i32); sig("mgProfileReset", None); sig("mgProfileKernels", i32)
    sig("mgProfileGet", i32, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), U64P)
    _lib = L
    return L


class ModgpuError(RuntimeError):
    pass


def check(status):
    if status != 0:
        raise ModgpuError("libmodgpu status %d: %s" % (status, lib().mgLastError().decode()))


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]
_libc.fopen.restype = C.c_void_p
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fclose.argtypes = [C.c_void_p]


class CFile:
    """FILE* for the reference-style functions that print to a FILE (modsetSummary etc.)."""

    def __init__(self, path, mode="w"):
        self.f = _libc.fopen(path.encode(), mode.encode())
        if not self.f:
            raise OSError("cannot open " + path)

    def __enter__(self):
        return C.c_void_p(self.f)

    def __exit__(self, *a):
        _libc.fclose(self.f)


# ------------------------------------------------------------------------------------------------
# Host-side mirror of the reference interface (same names / argument meaning).

def seqhashCreate(k, w, seed=17):
    """reference seqhash.c:20-37.  Invalid k/w make the C library die() exactly like the reference;
    here they raise ValueError first so a Python caller survives."""
    if k < 1 or k >= 32:
        raise ValueError("seqhash k %d must be between 1 and 32" % k)
    if w < 1:
        raise ValueError("seqhash w %d must be positive" % w)
    return lib().seqhashCreate(k, w, seed)


def modsetCreate(sh, bits, size=0):
    """reference modset.c:15-31"""
    if bits < 20 or bits > 34:
        raise ValueError("table bits %d must be between 20 and 34" % bits)
    if size >= (1 << bits) >> 2:
        raise ValueError("Modset size %u is too big for %d bits" % (size, bits))
    return lib().modsetCreate(sh, bits, size)


def iterate(sh, bases, minimizer=False):
    """Drive modRCiterator/modRCnext (or the minimizer pair) over one read, as the reference's
    callers do (modutils.c:22-29).  bases: uint8 array of 0..3."""
    L = lib()
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    mk, nx = (L.minimizerRCiterator, L.minimizerRCnext) if minimizer else (L.modRCiterator, L.modRCnext)
    it = mk(sh, bases.ctypes.data, len(bases))
    u = C.c_uint64(); p = C.c_int(); f = C.c_bool()
    ks, ps, fs = [], [], []
    while nx(it, C.byref(u), C.byref(p), C.byref(f)):
        ks.append(u.value); ps.append(p.value); fs.append(int(f.value))
    L.mgSeqhashRCiteratorDestroy(it)
    return np.array(ks, np.uint64), np.array(ps, np.int32), np.array(fs, np.uint8)


def scan_batch(sh, bases, offsets):
    """seqhashScanBatch: all modimizers of a batch of reads in (read,pos) order.
    Returns (kmer u64[], pos i32[], isF u8[], survStart i64[nReads+1])."""
    L = lib()
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n_reads = len(offsets) - 1
    pk, pp, pf, ps = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n = L.seqhashScanBatch(sh, bases.ctypes.data, offsets.ctypes.data, n_reads,
                           C.byref(pk), C.byref(pp), C.byref(pf), C.byref(ps))
    if n < 0:
        raise ModgpuError("seqhashScanBatch failed: " + L.mgLastError().decode())

    def take(ptr, ctype, count, dtype):
        a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (max(count, 1),))[:count].astype(dtype, copy=True)
        _libc.free(ptr)
        return a
    kmer = take(pk, C.c_uint64, n, np.uint64)
    pos = take(pp, C.c_int, n, np.int32)
    isf = take(pf, C.c_bool, n, np.uint8)
    st = take(ps, C.c_int64, n_reads + 1, np.int64)
    return kmer, pos, isf, st


def minimizer_batch(sh, bases, offsets):
    """seqhashMinimizerBatch: what minimizerRCnext returns for every read of a batch, reads in order.
    Returns (hash u64[], pos i32[], isF u8[], start i64[nReads+1])."""
    L = lib()
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n_reads = len(offsets) - 1
    pk, pp, pf, ps = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n = L.seqhashMinimizerBatch(sh, bases.ctypes.data, offsets.ctypes.data, n_reads,
                                C.byref(pk), C.byref(pp), C.byref(pf), C.byref(ps))
    if n < 0:
        raise ModgpuError("seqhashMinimizerBatch failed: " + L.mgLastError().decode())

    def take(ptr, ctype, count, dtype):
        a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (max(count, 1),))[:count].astype(dtype, copy=True)
        _libc.free(ptr)
        return a
    return (take(pk, C.c_uint64, n, np.uint64), take(pp, C.c_int, n, np.int32), take(pf, C.c_bool, n, np.uint8),
            take(ps, C.c_int64, n_reads + 1, np.int64))


class DeviceBuffer:
    """A raw device allocation owned through the C ABI (no torch needed)."""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        check(lib().mgDeviceAlloc(C.byref(self.ptr), self.nbytes))

    @classmethod
    def from_numpy(cls, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(max(arr.nbytes, 16))
        if arr.nbytes:
            check(lib().mgMemcpyH2D(b.ptr, arr.ctypes.data, arr.nbytes, None))
            check(lib().mgStreamSynchronize(None))
        return b

    def to_numpy(self, dtype, count):
        out = np.empty(count, dtype)
        if out.nbytes:
            check(lib().mgMemcpyD2H(out.ctypes.data, self.ptr, out.nbytes, None))
        return out

    def free(self):
        if self.ptr:
            lib().mgDeviceFree(self.ptr); self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pack_host(bases):
    """mgPackHost: bytes 0..3 -> 2-bit packed uint32 words (first base in the top bits)."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    words = np.zeros(lib().mgPackedWords(len(bases)), np.uint32)
    lib().mgPackHost(bases.ctypes.data, len(bases), words.ctypes.data)
    return words


def modset_arrays(ms):
    """Host view (copies) of value/depth/info for entries 0..max of a Modset*."""
    m = ms.contents
    n = m.max + 1
    return (np.ctypeslib.as_array(m.value, (n,)).copy(),
            np.ctypeslib.as_array(m.depth, (n,)).copy(),
            np.ctypeslib.as_array(m.info, (n,)).copy())


def add_sequence_batch(ms, bases, offsets):
    """mgAddSequenceBatch: modutils.c:19-31 over a batch of reads (GPU). Returns total hashes."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = lib().mgAddSequenceBatch(ms, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1)
    if n < 0:
        raise ModgpuError("mgAddSequenceBatch failed: " + lib().mgLastError().decode())
    return n


def report_depths(ms, others, path):
    """mgReportDepths: modutils -d (modutils.c:65-77) into the file `path`; others: a list of Modset*.  Their device tables stay resident
    (mgModsetDeviceRelease releases one)."""
    arr = (C.POINTER(Modset) * max(len(others), 1))(*others)
    with CFile(path, "w") as f:
        rc = lib().mgReportDepths(ms, arr, len(others), f)
    if rc:
        raise ModgpuError("mgReportDepths failed: " + lib().mgLastError().decode())


def refpaint_file(ms, path, out_path):
    """mgRefPaintFile: modutils -P (modutils.c:260-273) on the FASTA / FASTQ file `path`, its lines into the file `out_path`."""
    with CFile(out_path, "w") as f:
        rc = lib().mgRefPaintFile(ms, path.encode(), f)
    if rc:
        raise ModgpuError("mgRefPaintFile failed: " + lib().mgLastError().decode())


def refpaint(ms, bases, offsets, names, out_path):
    """mgRefPaint: modutils -P on records already in memory (bases 0..3, offsets[n+1], names: list of str) into `out_path`."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    nm = (C.c_char_p * max(n, 1))(*[x.encode() for x in names])
    with CFile(out_path, "w") as f:
        rc = lib().mgRefPaint(ms, bases.ctypes.data, offsets.ctypes.data, n, nm, f)
    if rc:
        raise ModgpuError("mgRefPaint failed: " + lib().mgLastError().decode())


def write_text_device(ms, path):
    """mgModsetWriteTextDevice: modutils -wt (modutils.c:191-199) into the file `path`, the lines formatted on the device."""
    with CFile(path, "w") as f:
        rc = lib().mgModsetWriteTextDevice(ms, f)
    if rc:
        raise ModgpuError("mgModsetWriteTextDevice failed: " + lib().mgLastError().decode())


def read_text(path):
    """mgModsetReadText: modutils -rt (modutils.c:169-190): the Modset* the text table `path` describes (the caller destroys it and its
    hasher).  read_text_path() tells which way it was read: 0 parsed on the device, 1 parsed on the host and inserted on the device,
    2 built on the host."""
    ms = lib().mgModsetReadText(path.encode())
    if not ms:
        raise ModgpuError("mgModsetReadText failed: " + lib().mgLastError().decode())
    return ms


def read_text_path():
    return lib().mgModsetReadTextPath()


def add_sequence_file_10x(ms, path, out_path, mode="w"):
    """mgAddSequenceFile10x: modutils -x (modutils.c:33-51 with is10x) on the file `path`, its line into `out_path`.  Returns
    mgAdd10xDiag: (batches trimmed on the device, records with an odd number, bases dropped, 1 if the host parser took a part)."""
    with CFile(out_path, mode) as f:
        rc = lib().mgAddSequenceFile10x(ms, path.encode(), f)
    if rc:
        raise ModgpuError("mgAddSequenceFile10x failed: " + lib().mgLastError().decode())
    out = (C.c_uint64 * 4)()
    lib().mgAdd10xDiag(out)
    return tuple(int(x) for x in out)


def set_copy(ms, copy1min, copy2min, copy_m_min):
    """mgModsetSetCopy: modutils -s (modutils.c:205-212).  Returns the path taken: 0 the device table, 1 the host loop."""
    if lib().mgModsetSetCopy(ms, copy1min, copy2min, copy_m_min):
        raise ModgpuError("mgModsetSetCopy failed: " + lib().mgLastError().decode())
    return lib().mgModsetSetCopyPath()


def set_copy_m(ms, copy_m_min):
    """mgModsetSetCopyM: modutils -sM (modutils.c:215-217).  Returns the path taken: 0 the device table, 1 the host loop."""
    if lib().mgModsetSetCopyM(ms, copy_m_min):
        raise ModgpuError("mgModsetSetCopyM failed: " + lib().mgLastError().decode())
    return lib().mgModsetSetCopyPath()


def summary_device(ms, path, mode="w"):
    """mgModsetSummaryDevice: modsetSummary's lines into the file `path`, counted on the device where the set has a table there."""
    with CFile(path, mode) as f:
        rc = lib().mgModsetSummaryDevice(ms, f)
    if rc:
        raise ModgpuError("mgModsetSummaryDevice failed: " + lib().mgLastError().decode())
    return open(path).read()


def readset_clean_mods(rs, path):
    """mgReadsetCleanMods: modasm -C (modasm.c:514-555) on the MgReadset* `rs`, its line into the file `path`.  Returns the path taken:
    0 the device, 1 the host loops."""
    with CFile(path, "w") as f:
        rc = lib().mgReadsetCleanMods(rs, f)
    if rc:
        raise ModgpuError("mgReadsetCleanMods failed: " + lib().mgLastError().decode())
    return lib().mgReadsetCleanModsPath()


def readset_properties(rs, path):
    """mgReadsetProperties: modasm -P (modasm.c:912-952), its lines into the file `path`.  Returns the path taken as above."""
    with CFile(path, "w") as f:
        rc = lib().mgReadsetProperties(rs, f)
    if rc:
        raise ModgpuError("mgReadsetProperties failed: " + lib().mgLastError().decode())
    return lib().mgReadsetPropertiesPath()


def _overlaps_done(rc, what):
    if rc:
        raise ModgpuError("%s failed: %s" % (what, lib().mgLastError().decode()))
    return lib().mgReadsetOverlapsPath()


def readset_find_overlaps(rs, reads, level, f, want_lists=False):
    """mgReadsetFindOverlaps: findOverlaps (modasm.c:314-418) for the read numbers `reads` in order -- modasm -o1 i is one read at level 2 --
    its lines into the open CFile `f` (None: none).  Returns the path taken (0 the device, 1 the host loops), or with want_lists the lists
    as -b / -c see them: per query [(iy, nHit, nBadOrder, nBadFlip, flags)]."""
    reads = np.ascontiguousarray(reads, dtype=np.uint32)
    res = MgOverlaps()
    rc = lib().mgReadsetFindOverlaps(rs, reads.ctypes.data, len(reads), level, f, C.byref(res) if want_lists else None)
    path = _overlaps_done(rc, "mgReadsetFindOverlaps")
    if not want_lists:
        return path
    out = [[(int(res.iy[e]), int(res.nHit[e]), int(res.nBadOrder[e]), int(res.nBadFlip[e]), int(res.flags[e]))
            for e in range(int(res.start[q]), int(res.start[q + 1]))] for q in range(res.n)]
    lib().mgOverlapsFree(C.byref(res))
    return out


def readset_overlap_stats(rs, d, f):
    """mgReadsetOverlapStats: modasm -o2 d, the "RR" lines of reads d, 2d, .. into the open CFile `f`.  Returns the path taken."""
    return _overlaps_done(lib().mgReadsetOverlapStats(rs, d, f), "mgReadsetOverlapStats")


def readset_mark_bad_reads(rs, f):
    """mgReadsetMarkBadReads: modasm -b (markBadReads, modasm.c:1266-1322): rs.bad, the three "MB" lines into `f`.  Returns the path taken."""
    return _overlaps_done(lib().mgReadsetMarkBadReads(rs, f), "mgReadsetMarkBadReads")


def readset_mark_contained(rs, f):
    """mgReadsetMarkContained: modasm -c (markContained, modasm.c:1370-1394): rs.contained, the "MC" line into `f`.  Returns the path taken."""
    return _overlaps_done(lib().mgReadsetMarkContained(rs, f), "mgReadsetMarkContained")


def readset_overlaps_diag():
    """mgReadsetOverlapsDiag: (batches, candidates, pairs kept, pair-kernel launches) of the calling thread's last overlap call"""
    v = (C.c_uint64 * 4)()
    lib().mgReadsetOverlapsDiag(v)
    return tuple(int(x) for x in v)


def _rdna_done(rc, what):
    if rc:
        raise ModgpuError("%s failed: %s" % (what, lib().mgLastError().decode()))
    return lib().mgReadsetRdnaPath()


def readset_ref_flag(rs, ref_path, f):
    """mgReadsetRefFlagFile: modasm -R <ref> (refFlag, modasm.c:752-860), its five counting lines into the open CFile `f` (None: none).  Returns the
    path taken: 0 the device, 1 the host loops."""
    return _rdna_done(lib().mgReadsetRefFlagFile(rs, ref_path.encode(), f), "mgReadsetRefFlagFile")


def readset_ref_flag_hits(rs, index, pos, f):
    """mgReadsetRefFlagHits: the same from the reference sequences' hits in file order (mod index, position), misses left out"""
    index = np.ascontiguousarray(index, dtype=np.uint32)
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    assert len(index) == len(pos)
    return _rdna_done(lib().mgReadsetRefFlagHits(rs, index.ctypes.data, pos.ctypes.data, len(index), f), "mgReadsetRefFlagHits")


def readset_reset_bits(rs, op, f):
    """mgReadsetResetBits: modasm -rb op (resetBits, modasm.c:864-908), its line into `f`.  Returns the path taken."""
    return _rdna_done(lib().mgReadsetResetBits(rs, op, f), "mgReadsetResetBits")


def readset_test_mods(rs, min_depth, max_depth, f, y=None, z=None):
    """mgReadsetTestMods: modasm -T min max (testMods, modasm.c:595-748): the "RUN" line into `f`, the "YY-TEST" lines into the CFile `y` and the
    "ZZ-TEST" lines into `z` (None: not made).  Returns the path taken."""
    return _rdna_done(lib().mgReadsetTestMods(rs, min_depth, max_depth, y, z, f), "mgReadsetTestMods")


def readset_mod_info(rs):
    """mgReadsetModInfo: a numpy view (fields flags, rDNApos, nGood, nMod2, nBadLD, nSplit, nSplitLD) of the ms->max + 1 entries; None before -R.
    The view is of the library's array: it is replaced by the next -R or -T."""
    p = lib().mgReadsetModInfo(rs)
    if not p:
        return None
    dt = np.dtype([("flags", np.uint8), ("rDNApos", np.int32), ("nGood", np.int32), ("nMod2", np.int32), ("nBadLD", np.int32), ("nSplit", np.int32),
                   ("nSplitLD", np.int32)], align=True)
    assert dt.itemsize == C.sizeof(MgModInfo)
    n = rs.contents.ms.contents.max + 1
    return np.frombuffer((C.c_char * (n * dt.itemsize)).from_address(C.addressof(p.contents)), dtype=dt)


def readset_read_flags(rs):
    """mgReadsetReadFlags: Read.otherFlags of reads 0 .. nReads (entry 0 unused) as a numpy copy; bit 1 = isRDNA"""
    p = lib().mgReadsetReadFlags(rs)
    return np.ctypeslib.as_array(p, (rs.contents.nReads + 1,)).copy()


def readset_rdna_diag():
    """mgReadsetRdnaDiag: (batches, tested mods, visits, partner occurrences) of the calling thread's last -T"""
    v = (C.c_uint64 * 4)()
    lib().mgReadsetRdnaDiag(v)
    return tuple(int(x) for x in v)


def readset_rdna_grid():
    """mgReadsetRdnaGrid: (partner tiles, least share, greatest share, cells per count array) of the calling thread's last -T on the device"""
    v = (C.c_uint32 * 4)()
    lib().mgReadsetRdnaGrid(v)
    return tuple(int(x) for x in v)


def rep_ref_create(seq_path, mod_path, err_path=None):
    """mgRepRefCreate: modrep -R (modrep.c:27-63): the MgRepRef* of the one sequence of `seq_path` against the set `mod_path`; the "found"
    line into the file `err_path` if given.  Raises with the program's message otherwise.  Destroy with lib().mgRepRefDestroy."""
    if err_path is None:
        ref = lib().mgRepRefCreate(seq_path.encode(), mod_path.encode(), None)
    else:
        with CFile(err_path, "w") as f:
            ref = lib().mgRepRefCreate(seq_path.encode(), mod_path.encode(), f)
    if not ref:
        raise ModgpuError(lib().mgLastError().decode())
    return ref


def rep_ref_from_arrays(ms, bases, err_path=None):
    """mgRepRefFromArrays: modrep.c:43-54 on a sequence in memory (bases 0..3); ms stays the caller's."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    if err_path is None:
        ref = lib().mgRepRefFromArrays(ms, bases.ctypes.data, len(bases), None)
    else:
        with CFile(err_path, "w") as f:
            ref = lib().mgRepRefFromArrays(ms, bases.ctypes.data, len(bases), f)
    if not ref:
        raise ModgpuError(lib().mgLastError().decode())
    return ref


def _rep_result(res):
    """the arrays of an MgRepResult as numpy copies in a dict; frees the C arrays"""
    def arr(ptr, count, dtype):
        return np.ctypeslib.as_array(ptr, (max(count, 1),))[:count].astype(dtype, copy=True)
    n_hit = int(res.hitStart[res.nGood])
    out = dict(nRead=res.nRead, nBad=res.nBad, nGood=res.nGood, max=res.max, nMod=res.nMod, nDup=res.nDup, tDup=res.tDup, minMax=res.minMax,
               n=arr(res.n, res.nRead, np.int32), seqF=arr(res.seqF, res.nRead, np.int32), seqR=arr(res.seqR, res.nRead, np.int32),
               bad=arr(res.bad, res.nRead, np.uint8), isF=arr(res.isF, res.nRead, np.uint8),
               modN=arr(res.modN, res.max + 1, np.int32), modNPre=arr(res.modNPre, res.max + 1, np.int32),
               goodI=arr(res.goodI, res.nGood, np.int32), goodLen=arr(res.goodLen, res.nGood, np.int32),
               hitStart=arr(res.hitStart, res.nGood + 1, np.int64), hitK=arr(res.hitK, n_hit, np.int32), hitX=arr(res.hitX, n_hit, np.int32))
    lib().mgRepResultFree(C.byref(res))
    return out


def rep_analyze3_file(ref, seq_path, mod_path, out_path, err_path):
    """mgRepAnalyze3File: modrep -s3 (modrep.c:170-268): the BADREAD lines into the file `out_path`, the two summary lines into `err_path`.
    Returns the MgRepResult as a dict of numpy arrays and ints."""
    res = MgRepResult()
    with CFile(out_path, "w") as fo, CFile(err_path, "w") as fe:
        rc = lib().mgRepAnalyze3File(ref, seq_path.encode(), mod_path.encode(), fo, fe, C.byref(res))
    if rc:
        raise ModgpuError("mgRepAnalyze3File failed: " + lib().mgLastError().decode())
    return _rep_result(res)


def rep_run(ref, ms, batches, out_path, err_path):
    """mgRepRunBegin / mgRepRunAdd per (bases, offsets) of `batches` / mgRepRunFinish: modrep -s3 on reads in memory, lines as above.
    Returns the MgRepResult as a dict of numpy arrays and ints."""
    L = lib()
    run = L.mgRepRunBegin(ref, ms)
    if not run:
        raise ModgpuError("mgRepRunBegin failed: " + L.mgLastError().decode())
    res = MgRepResult()
    with CFile(out_path, "w") as fo, CFile(err_path, "w") as fe:
        rc = 0
        for bases, offsets in batches:
            bases = np.ascontiguousarray(bases, dtype=np.uint8)
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            rc = L.mgRepRunAdd(run, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1, fo)
            if rc:
                break
        msg = L.mgLastError().decode() if rc else ""
        rf = L.mgRepRunFinish(run, None if rc else fe, None if rc else C.byref(res))
    if rc or rf:
        raise ModgpuError("modrep -s3 failed: " + (msg or L.mgLastError().decode()))
    return _rep_result(res)


def _rep1_result(res):
    """the arrays of an MgRep1Result as numpy copies in a dict; frees the C arrays"""
    def arr(ptr, count, dtype):
        return np.ctypeslib.as_array(ptr, (max(count, 1),))[:count].astype(dtype, copy=True)
    m = res.max
    pre_s, post_s = arr(res.preStart, m + 2, np.int64), arr(res.postStart, m + 2, np.int64)
    hs = arr(res.hitStart, res.readsAfter + 1, np.int64)
    out = dict(nRead=res.nRead, nBad=res.nBad, nGood=res.nGood, max=m, nmod=np.array([list(row) for row in res.nmod], np.int32),
               readsBefore=res.readsBefore, readsAfter=res.readsAfter,
               modN=arr(res.modN, m + 1, np.int32), modNPre=arr(res.modNPre, m + 1, np.int32), modNPost=arr(res.modNPost, m + 1, np.int32),
               preStart=pre_s, postStart=post_s)
    for side, start in (("pre", pre_s), ("post", post_s)):
        for f in "KNX":
            out[side + f] = arr(getattr(res, side + f), int(start[-1]), np.int32)
    out.update(readI=arr(res.readI, res.readsAfter, np.int32), hitStart=hs, hitK=arr(res.hitK, int(hs[-1]), np.int32))
    lib().mgRep1ResultFree(C.byref(res))
    return out


def rep_analyze1_file(ref, seq_path, mod_path, out_path, err_path):
    """mgRepAnalyze1File: modrep -s1 (modrep.c:272-489): the NMOD / MOD / BLOCK / READ lines into the file `out_path`, the two stderr lines
    into `err_path`.  Returns the MgRep1Result as a dict of numpy arrays and ints; raises ModgpuError with the library's message."""
    res = MgRep1Result()
    with CFile(out_path, "w") as fo, CFile(err_path, "w") as fe:
        rc = lib().mgRepAnalyze1File(ref, seq_path.encode(), mod_path.encode(), fo, fe, C.byref(res))
    if rc:
        raise ModgpuError("mgRepAnalyze1File failed: " + lib().mgLastError().decode())
    return _rep1_result(res)


def rep_run1(ref, ms, batches, out_path, err_path):
    """mgRepRunBegin / mgRepRunAdd (out = 0) per (bases, offsets) of `batches` / mgRepRunFinish1: modrep -s1 on reads in memory"""
    L = lib()
    run = L.mgRepRunBegin(ref, ms)
    if not run:
        raise ModgpuError("mgRepRunBegin failed: " + L.mgLastError().decode())
    res = MgRep1Result()
    with CFile(out_path, "w") as fo, CFile(err_path, "w") as fe:
        rc = 0
        for bases, offsets in batches:
            bases = np.ascontiguousarray(bases, dtype=np.uint8)
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            rc = L.mgRepRunAdd(run, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1, None)
            if rc:
                break
        msg = L.mgLastError().decode() if rc else ""
        rf = L.mgRepRunFinish(run, None, None) if rc else L.mgRepRunFinish1(run, fo, fe, C.byref(res))
    if rc or rf:
        raise ModgpuError("modrep -s1 failed: " + (msg or L.mgLastError().decode()))
    return _rep1_result(res)


def rep_analyze1_hits(max_, k, read_i, hit_start, hit_k, hit_x, out_path, err_path):
    """mgRepAnalyze1Hits: the end of a -s1 file (modrep.c:354-480) on hit lists in memory; lines and result as rep_analyze1_file"""
    read_i = np.ascontiguousarray(read_i, dtype=np.int32)
    hit_start = np.ascontiguousarray(hit_start, dtype=np.uint64)
    hit_k = np.ascontiguousarray(hit_k, dtype=np.int32)
    hit_x = np.ascontiguousarray(hit_x, dtype=np.int32)
    res = MgRep1Result()
    with CFile(out_path, "w") as fo, CFile(err_path, "w") as fe:
        rc = lib().mgRepAnalyze1Hits(max_, k, len(read_i), read_i.ctypes.data, hit_start.ctypes.data, hit_k.ctypes.data, hit_x.ctypes.data, fo, fe, C.byref(res))
    if rc:
        raise ModgpuError("mgRepAnalyze1Hits failed: " + lib().mgLastError().decode())
    return _rep1_result(res)


def rep_count2(ref, bases, offsets, counts=None):
    """mgRepCount2: modrep -s2's four counts (modrep.c:520-535) of a batch added to `counts` (a list of 4 ints; None: zeros); returns the list"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    c = (C.c_int * 4)(*(counts or [0, 0, 0, 0]))
    if lib().mgRepCount2(ref, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1, c):
        raise ModgpuError("mgRepCount2 failed: " + lib().mgLastError().decode())
    return list(c)


def rep_analyze2_file(ref, seq_path, mod_path, out_path):
    """mgRepAnalyze2File: modrep -s2 (modrep.c:498-539): its one line into the file `out_path`; returns the four counts"""
    c = (C.c_int * 4)()
    with CFile(out_path, "w") as fo:
        rc = lib().mgRepAnalyze2File(ref, seq_path.encode(), mod_path.encode(), fo, c)
    if rc:
        raise ModgpuError("mgRepAnalyze2File failed: " + lib().mgLastError().decode())
    return list(c)


COMP_BASES, COMP_QUALS, COMP_LENGTHS = 1, 2, 4      # include/modgpu.h: composition's -b, -q, -l


def _composition(call, what):
    """run `call (out FILE *, err FILE *, result *)`; (stdout text, stderr text, the MgComposition as a dict of ints and numpy arrays)"""
    import tempfile
    res = MgComposition()
    with tempfile.TemporaryDirectory(prefix="modgpu_comp_") as d:
        po, pe = os.path.join(d, "out"), os.path.join(d, "err")
        with CFile(po, "w") as fo, CFile(pe, "w") as fe:
            rc = call(fo, fe, C.byref(res))
        out, err = open(po, "rb").read(), open(pe, "rb").read()
    def arr(ptr, count, dtype):
        return np.ctypeslib.as_array(ptr, (count,)).astype(dtype, copy=True) if count and ptr else np.zeros(0, dtype)
    r = dict(type=res.type, nSeq=res.nSeq, totLen=res.totLen, lenMin=res.lenMin, lenMax=res.lenMax,
             base=np.array(res.base, np.uint64), qual=np.array(res.qual, np.uint64),
             binCount=arr(res.binCount, res.nBins, np.int32), binSum=arr(res.binSum, res.nBins, np.uint64))
    lib().mgCompositionFree(C.byref(res))
    if rc:
        e = ModgpuError(what + " failed: " + lib().mgLastError().decode())
        e.out, e.err, e.result = out, err, r
        raise e
    return out.decode("latin-1"), err.decode("latin-1"), r


def composition_file(path, flags=0):
    """mgCompositionFile: the reference's `composition [-b] [-q] [-l] file` (flags: COMP_BASES | COMP_QUALS | COMP_LENGTHS) counted on the
    device.  Returns (stdout text, stderr text, result dict: type, nSeq, totLen, lenMin, lenMax, base[256], qual[256], binCount, binSum);
    raises ModgpuError with the library's message (its .out, .err and .result hold what the call left)."""
    return _composition(lambda fo, fe, res: lib().mgCompositionFile(os.fsencode(path), flags, fo, fe, res), "mgCompositionFile")


def composition_text(text, flags=0):
    """mgCompositionText: the same on the file's bytes in memory (bytes or a uint8 array)"""
    buf = np.frombuffer(bytes(text), np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
    return _composition(lambda fo, fe, res: lib().mgCompositionText(buf.ctypes.data if len(buf) else None, len(buf), flags, fo, fe, res), "mgCompositionText")


def composition_diag():
    """mgCompositionDiag: dict(windows, tiles, crossed, launches) of the calling thread's last composition call"""
    v = (C.c_uint64 * 4)()
    lib().mgCompositionDiag(v)
    return dict(zip(("windows", "tiles", "crossed", "launches"), (int(x) for x in v)))


SEQ_FASTA, SEQ_FASTQ, SEQ_HOCO = 1, 2, 4      # include/modgpu.h: seqconvert -fa, -fq; seqhoco


def _seq_convert_result(res):
    return {n: int(getattr(res, n)) for n, _ in MgSeqConvert._fields_}


def seq_convert_file(in_path, out_path, flags=0):
    """mgSeqConvertFile: the reference's `seqconvert -fa|-fq -o out in` (flags: SEQ_FASTA or SEQ_FASTQ; without one the type is out's .fa /
    .fq suffix) or, with SEQ_HOCO, `seqhoco in` written to out, rewritten on the device.  Returns (stderr text, result dict); raises
    ModgpuError with the library's message (its .err and .result hold what the call left)."""
    import tempfile
    res = MgSeqConvert()
    with tempfile.TemporaryDirectory(prefix="modgpu_conv_") as d:
        pe = os.path.join(d, "err")
        with CFile(pe, "w") as fe:
            rc = lib().mgSeqConvertFile(os.fsencode(in_path), os.fsencode(out_path), flags, fe, C.byref(res))
        err = open(pe, "rb").read()
    if rc:
        e = ModgpuError("mgSeqConvertFile failed: " + lib().mgLastError().decode("latin-1"))
        e.err, e.result = err, _seq_convert_result(res)
        raise e
    return err.decode("latin-1"), _seq_convert_result(res)


def seq_convert_text(data, flags):
    """mgSeqConvertText: the same on the file's bytes in memory (bytes or a uint8 array).  Returns (output bytes, stderr text, result dict)"""
    import tempfile
    buf = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
    res = MgSeqConvert()
    with tempfile.TemporaryDirectory(prefix="modgpu_conv_") as d:
        po, pe = os.path.join(d, "out"), os.path.join(d, "err")
        with CFile(po, "w") as fo, CFile(pe, "w") as fe:
            rc = lib().mgSeqConvertText(buf.ctypes.data if len(buf) else None, len(buf), flags, fo, fe, C.byref(res))
        out, err = open(po, "rb").read(), open(pe, "rb").read()
    if rc:
        e = ModgpuError("mgSeqConvertText failed: " + lib().mgLastError().decode("latin-1"))
        e.out, e.err, e.result = out, err, _seq_convert_result(res)
        raise e
    return out, err.decode("latin-1"), _seq_convert_result(res)


def seq_convert_diag():
    """mgSeqConvertDiag: dict(windows, tiles, crossed, launches) of the calling thread's last conversion"""
    v = (C.c_uint64 * 4)()
    lib().mgSeqConvertDiag(v)
    return dict(zip(("windows", "tiles", "crossed", "launches"), (int(x) for x in v)))


INFLATE_STATUS = ("ok", "input exhausted", "bad block type", "stored LEN/NLEN mismatch", "bad code lengths", "invalid symbol",
                  "distance beyond the start", "output longer or shorter than stated", "CRC mismatch")      # include/modgpu.h
INFLATE_STATS = ("stored", "fixed", "dynamic", "litlen_bits", "distance", "match", "dist_bits", "symbols")
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")      # bgzip's end marker: an empty member


def bgzf_member(payload, text_len, crc):
    """one BGZF member around a raw-deflate payload: the gzip header with the 'BC' extra field (the member's size - 1), CRC-32 and length"""
    import struct
    if len(payload) + 26 > 65536:
        raise ValueError("a BGZF member holds at most 65510 compressed bytes")
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(payload) + 25) + payload + struct.pack("<II", crc, text_len)


def bgzf_bytes(data, block=65280, level=6, eof=True, threads=1):
    """blocked gzip (BGZF) as bgzip writes it, from Python's zlib: members of `block` text bytes (65280 is bgzip's), then the empty end marker;
    threads > 1: the members are deflated by that many threads (zlib releases the interpreter lock)"""
    import zlib
    data = memoryview(bytes(data) if not isinstance(data, (bytes, memoryview)) else data)

    def one(i):
        ch = bytes(data[i:i + block])
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        pay = c.compress(ch) + c.flush()
        if len(pay) + 26 > 65536:                     # text that deflate cannot shrink: stored, as bgzip falls back to
            c = zlib.compressobj(0, zlib.DEFLATED, -15)
            pay = c.compress(ch) + c.flush()
        return bgzf_member(pay, len(ch), zlib.crc32(ch))
    starts = range(0, len(data), block)
    if threads > 1:
        from multiprocessing.pool import ThreadPool
        with ThreadPool(threads) as pool:
            out = pool.map(one, starts, chunksize=64)
    else:
        out = [one(i) for i in starts]
    if eof:
        out.append(BGZF_EOF)
    return b"".join(out)


def bgzf_members(blob):
    """the members of a BGZF blob as mgInflateMembersDevice takes them: [(payload offset, payload length, text offset, text length, crc)]"""
    import struct
    out, at, u = [], 0, 0
    while at < len(blob):
        xlen, = struct.unpack_from("<H", blob, at + 10)
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        crc, n = struct.unpack_from("<II", blob, at + size - 8)
        out.append((at + 12 + xlen, size - 12 - xlen - 8, u, n, crc))
        at += size; u += n
    return out


def inflate_member_host(payload, text_len, crc, guard=64):
    """mgInflateMemberHost: one raw-deflate payload through the decoder's host compile.  Returns (status, text bytes, stats dict, guards intact):
    the output range lies between `guard` bytes of 0xA5 on both sides, and so does a copy of the payload."""
    payload = bytes(payload)
    comp = np.full(len(payload) + 2 * guard, 0xA5, np.uint8)
    comp[guard:guard + len(payload)] = np.frombuffer(payload, np.uint8)
    out = np.full(text_len + 2 * guard, 0xA5, np.uint8)
    st = C.c_uint32(99)
    stats = (C.c_uint64 * 8)()
    if lib().mgInflateMemberHost(comp.ctypes.data + guard, len(payload), out.ctypes.data + guard, text_len, crc, C.byref(st), stats):
        raise ModgpuError("mgInflateMemberHost failed: " + lib().mgLastError().decode("latin-1"))
    intact = bool((out[:guard] == 0xA5).all() and (out[guard + text_len:] == 0xA5).all())
    return int(st.value), out[guard:guard + text_len].tobytes(), dict(zip(INFLATE_STATS, (int(x) for x in stats))), intact


def inflate_members_device(comp, members, out_bytes, fill=0xA5):
    """mgInflateMembersDevice: `comp` (bytes) to the device, the members [(cOff, cLen, uOff, uLen, crc)] inflated into a device buffer of out_bytes
    bytes preset to `fill`.  Returns (the whole output buffer as a uint8 array, statuses as a uint32 array, nBad); raises ModgpuError on a refusal."""
    comp = np.frombuffer(bytes(comp), np.uint8)
    n = len(members)
    tab = (MgGzMember * max(n, 1))()
    for i, (c_off, c_len, u_off, u_len, crc) in enumerate(members):
        tab[i] = MgGzMember(c_off, u_off, c_len, u_len, crc, 0)
    d_comp, d_out = DeviceBuffer.from_numpy(comp), DeviceBuffer(max(out_bytes, 16))
    try:
        check(lib().mgMemsetD(d_out.ptr, fill, d_out.nbytes, None)); check(lib().mgStreamSynchronize(None))
        status = np.full(max(n, 1), 99, np.uint32)
        bad = C.c_uint32(0)
        rc = lib().mgInflateMembersDevice(d_comp.ptr, len(comp), tab, n, d_out.ptr, out_bytes, status.ctypes.data, C.byref(bad), None)
        if rc:
            e = ModgpuError("mgInflateMembersDevice failed: " + lib().mgLastError().decode("latin-1"))
            e.status = rc
            raise e
        return d_out.to_numpy(np.uint8, out_bytes), status[:n], int(bad.value)
    finally:
        d_comp.free(); d_out.free()


def inflate_diag():
    """mgInflateDiag: dict(members, uploaded, text, launches) of the calling thread's last call that could inflate on the device"""
    v = (C.c_uint64 * 4)()
    lib().mgInflateDiag(v)
    return dict(zip(("members", "uploaded", "text", "launches"), (int(x) for x in v)))


def text_file_diag():
    """mgTextFileDiag: dict(path, windows, text, handed_over) of the calling thread's last file call: path 0 = the host parser from the
    start, 1 = the device parser over plain text, 2 = over blocked gzip inflated on the device, 3 = over ordinary gzip inflated on the device"""
    v = (C.c_uint64 * 4)()
    lib().mgTextFileDiag(v)
    return dict(zip(("path", "windows", "text", "handed_over"), (int(x) for x in v)))


def bgzf_inflate_file(in_path, out_path):
    """mgBgzfInflateFile: `bgzip -d` on the device.  True; False if the file is not BGZF from end to end (nothing is written); raises ModgpuError"""
    rc = lib().mgBgzfInflateFile(os.fsencode(in_path), os.fsencode(out_path), None)
    if rc == -2:
        return False
    if rc:
        raise ModgpuError("mgBgzfInflateFile failed: " + lib().mgLastError().decode("latin-1"))
    return True


GUNZIP_STATUS = INFLATE_STATUS + ("a chunk of more than 2^28 symbols", "not a gzip header")
GUNZIP_DIAG = ("speculated", "confirmed", "discarded", "folded", "batches", "members", "retries", "launches")      # include/modgpu.h


def gunzip_host(blob, chunk_bytes, batch_chunks, symbols_per_chunk, cap, guard=64):
    """mgGunzipHost: a gzip file's bytes through the host compile of the device's pipeline.  Returns (status, text bytes, diag dict, guards intact):
    the output range of `cap` bytes lies between `guard` bytes of 0xA5 on both sides, and so does a copy of the file."""
    blob = bytes(blob)
    comp = np.full(len(blob) + 2 * guard, 0xA5, np.uint8)
    comp[guard:guard + len(blob)] = np.frombuffer(blob, np.uint8)
    out = np.full(cap + 2 * guard, 0xA5, np.uint8)
    st, n = C.c_uint32(99), C.c_uint64(0)
    diag = (C.c_uint64 * 8)()
    if lib().mgGunzipHost(comp.ctypes.data + guard, len(blob), chunk_bytes, batch_chunks, symbols_per_chunk, out.ctypes.data + guard, cap, C.byref(n), C.byref(st), diag):
        raise ModgpuError("mgGunzipHost failed: " + lib().mgLastError().decode("latin-1"))
    intact = bool((out[:guard] == 0xA5).all() and (out[guard + cap:] == 0xA5).all())
    return int(st.value), out[guard:guard + int(n.value)].tobytes(), dict(zip(GUNZIP_DIAG, (int(x) for x in diag))), intact


def gunzip_diag():
    """mgGunzipDiag: dict(speculated, confirmed, discarded, folded, batches, members, retries, launches) of the calling thread's last call that could
    inflate ordinary gzip on the device"""
    v = (C.c_uint64 * 8)()
    lib().mgGunzipDiag(v)
    return dict(zip(GUNZIP_DIAG, (int(x) for x in v)))


def gzip_src_diag():
    """mgGzipSrcDiag: dict(uploaded, refills, peak, bound) of the calling thread's last file call that walked an ordinary gzip file once (the text
    parser: path 3): compressed bytes uploaded, the times the resident range took bytes up, the most compressed bytes resident at once, the bound on them"""
    v = (C.c_uint64 * 4)()
    lib().mgGzipSrcDiag(v)
    return dict(zip(("uploaded", "refills", "peak", "bound"), (int(x) for x in v)))


def gzip_inflate_file(in_path, out_path):
    """mgGzipInflateFile: `gzip -dc` on the device.  True; False if the file is not ordinary gzip (nothing is written); raises ModgpuError"""
    rc = lib().mgGzipInflateFile(os.fsencode(in_path), os.fsencode(out_path), None)
    if rc == -2:
        return False
    if rc:
        raise ModgpuError("mgGzipInflateFile failed: " + lib().mgLastError().decode("latin-1"))
    return True


DEFLATE_STATS = ("kind", "literals", "matches", "match", "distance", "litlen_bits", "dist_bits", "bits")      # include/modgpu.h
BGZF_BLOCK = 65280                                    # text bytes of a member, at most: bgzip's


def deflate_block_host(text, guard=64):
    """mgDeflateBlockHost: one block of at most 65280 bytes through the encoder's host compile.  Returns (member bytes, stats dict, guards intact):
    the 65536-byte slot lies between `guard` bytes of 0xA5 on both sides, and so does a copy of the text."""
    text = bytes(text)
    src = np.full(len(text) + 2 * guard, 0xA5, np.uint8)
    src[guard:guard + len(text)] = np.frombuffer(text, np.uint8)
    keep = src.copy()
    out = np.full(65536 + 2 * guard, 0xA5, np.uint8)
    n = C.c_uint32(0)
    stats = (C.c_uint64 * 8)()
    if lib().mgDeflateBlockHost(src.ctypes.data + guard, len(text), out.ctypes.data + guard, C.byref(n), stats):
        raise ModgpuError("mgDeflateBlockHost failed: " + lib().mgLastError().decode("latin-1"))
    intact = bool((out[:guard] == 0xA5).all() and (out[guard + 65536:] == 0xA5).all() and (src == keep).all())
    return out[guard:guard + int(n.value)].tobytes(), dict(zip(DEFLATE_STATS, (int(x) for x in stats))), intact


def deflate_blocks_device(text, blocks, out_bytes=None, guard=4096, fill=0xA5):
    """mgDeflateBlocksDevice: `text` (bytes) to the device, its ranges [(offset, length)] deflated into BGZF members that are packed from the first
    byte of a device buffer of out_bytes bytes (default 65536 a block) with `guard` bytes preset to `fill` behind it.  Returns (the packed members as
    bytes, memberOff as a list of n + 1, guard intact); raises ModgpuError (.status) on a refusal."""
    data = np.frombuffer(bytes(text), np.uint8)
    n = len(blocks)
    out_bytes = 65536 * n if out_bytes is None else out_bytes
    tab = (MgGzBlock * max(n, 1))()
    for i, (off, length) in enumerate(blocks):
        tab[i] = MgGzBlock(off, length, 0)
    d_text, d_out = DeviceBuffer.from_numpy(data if len(data) else np.zeros(1, np.uint8)), DeviceBuffer(max(out_bytes, 16) + guard)
    try:
        check(lib().mgMemsetD(d_out.ptr, fill, d_out.nbytes, None)); check(lib().mgStreamSynchronize(None))
        off = (C.c_uint64 * (n + 1))()
        rc = lib().mgDeflateBlocksDevice(d_text.ptr, len(data), tab, n, d_out.ptr, out_bytes, off, None)
        if rc:
            e = ModgpuError("mgDeflateBlocksDevice failed: " + lib().mgLastError().decode("latin-1"))
            e.status = rc
            raise e
        whole = d_out.to_numpy(np.uint8, d_out.nbytes)
        end = int(off[n])
        return whole[:end].tobytes(), [int(x) for x in off], bool((whole[end:] == fill).all())
    finally:
        d_text.free(); d_out.free()


def deflate_diag():
    """mgDeflateDiag: dict(blocks, text, file, launches) of the calling thread's last call that could deflate on the device"""
    v = (C.c_uint64 * 4)()
    lib().mgDeflateDiag(v)
    return dict(zip(("blocks", "text", "file", "launches"), (int(x) for x in v)))


def bgzf_deflate_file(in_path, out_path):
    """mgBgzfDeflateFile: `bgzip` on the device: any regular file to out_path as BGZF (knobs(BGZF_BLOCK=n): n text bytes a member); raises ModgpuError"""
    if lib().mgBgzfDeflateFile(os.fsencode(in_path), os.fsencode(out_path), None):
        raise ModgpuError("mgBgzfDeflateFile failed: " + lib().mgLastError().decode("latin-1"))


def seqconvert_file_bgzf(in_path, out_path, flags=0):
    """mgSeqConvertFileBgzf: seq_convert_file with the output deflated on the device and written as BGZF, whatever out_path's suffix (the type may
    come from a .fa / .fq before .gz or .bgz).  Returns (stderr text, result dict); raises ModgpuError as seq_convert_file does."""
    import tempfile
    res = MgSeqConvert()
    with tempfile.TemporaryDirectory(prefix="modgpu_conv_") as d:
        pe = os.path.join(d, "err")
        with CFile(pe, "w") as fe:
            rc = lib().mgSeqConvertFileBgzf(os.fsencode(in_path), os.fsencode(out_path), flags, fe, C.byref(res))
        err = open(pe, "rb").read()
    if rc:
        e = ModgpuError("mgSeqConvertFileBgzf failed: " + lib().mgLastError().decode("latin-1"))
        e.err, e.result = err, _seq_convert_result(res)
        raise e
    return err.decode("latin-1"), _seq_convert_result(res)


def rep1_diag():
    """mgRep1Diag: dict(builds, links, entries, runs, dropped, stale, kernels) of the calling thread's last -s1 end"""
    v = (C.c_uint64 * 8)()
    lib().mgRep1Diag(v)
    return dict(zip(("builds", "links", "entries", "runs", "dropped", "stale", "kernels"), (int(x) for x in v)))
