// hip_engine_kb.cpp -- the parts of the engine around the hot path that change or persist the knowledge base:
// permanent<->compact id maps, quiz registry slots, .kb files, and the maintenance-mode operations.
// Reference: PqaCore/PermanentIdManager.cpp, PqaCore/BaseEngine.cpp:124-215,323-385,704-873,
// PqaCore/CpuEngine.cpp:468-658,664-688, PqaCore/PqaEngineBaseFactory.cpp:44-83.  Host bookkeeping is the reference's;
// the cube itself stays on the device and is edited there (kb_kernels.hip).
#include "hip_engine_internal.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

namespace pqa {

namespace {

template <typename T>
hipError_t Upload(T **dst, const std::vector<T> &src, hipStream_t stream) {
  *dst = nullptr;
  if (src.empty()) return hipSuccess;
  hipError_t e = hipMalloc(dst, src.size() * sizeof(T));
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, stream);
}

}  // namespace

Error FileErr(const char *path, const char *msg) {
  return Error::MakeP(ErrCode::FileOp, std::string("filePath=[") + path + "]", msg);
}

// ------------------------------------------------------------------------------------------------------------------
// IdLedger: compact slot <-> permanent id (hip_engine.h).  What callers and files observe follows the reference's
// PermanentIdManager; see the class comment for the structure.
// ------------------------------------------------------------------------------------------------------------------
size_t IdLedger::LowerBound(int64_t permanent) const {
  size_t lo = 0, hi = _byPerm.size();
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (_byPerm[mid].permanent < permanent) lo = mid + 1; else hi = mid;
  }
  return lo;
}

int64_t IdLedger::SlotOf(int64_t permanent) const {
  const size_t at = LowerBound(permanent);
  if (at == _byPerm.size() || _byPerm[at].permanent != permanent || !Live(_byPerm[at])) return kNone;
  return _byPerm[at].slot;
}

// Records that `slot` now carries `permanent` (the forward table is already written).  A leftover entry of the same id -- its
// slot was vacated earlier -- is taken over; otherwise the entry goes where the order puts it, which for a freshly issued id is
// the end.
void IdLedger::Enter(int64_t permanent, int64_t slot) {
  if (_byPerm.empty() || _byPerm.back().permanent < permanent) { _byPerm.push_back(Back{permanent, slot}); return; }
  const size_t at = LowerBound(permanent);
  if (at < _byPerm.size() && _byPerm[at].permanent == permanent) _byPerm[at].slot = slot;
  else _byPerm.insert(_byPerm.begin() + (ptrdiff_t)at, Back{permanent, slot});
}

void IdLedger::Rebuild() {
  _byPerm.clear();
  _live = 0;
  for (int64_t slot = 0; slot < (int64_t)_permOf.size(); slot++)
    if (_permOf[(size_t)slot] != kNone) { _byPerm.push_back(Back{_permOf[(size_t)slot], slot}); _live++; }
  std::sort(_byPerm.begin(), _byPerm.end(), [](const Back &x, const Back &y) { return x.permanent < y.permanent; });
}

bool IdLedger::Write(FILE *f, bool withoutSlots) const {
  const int64_t header[2] = {_issueNext, withoutSlots ? 0 : (int64_t)_permOf.size()};
  if (std::fwrite(header, sizeof(header), 1, f) != 1) return false;
  return header[1] == 0 || std::fwrite(_permOf.data(), sizeof(int64_t), (size_t)header[1], f) == (size_t)header[1];
}

bool IdLedger::Read(FILE *f) {
  int64_t header[2];
  if (std::fread(header, sizeof(header), 1, f) != 1 || header[1] < 0) return false;
  std::vector<int64_t> table((size_t)header[1]);
  if (header[1] > 0 && std::fread(table.data(), sizeof(int64_t), table.size(), f) != table.size()) return false;
  _issueNext = header[0];
  _permOf.swap(table);
  Rebuild();
  return true;
}

bool IdLedger::RaiseFloor(int64_t bound) {
  if (bound < _issueNext) return false;
  _issueNext = bound + 1;
  return true;
}

bool IdLedger::Vacate(int64_t slot) {
  if (!InRange(slot) || _permOf[(size_t)slot] == kNone) return false;
  _permOf[(size_t)slot] = kNone;     // its entry in _byPerm no longer agrees with the table: a leftover from here on
  _live--;
  if (_byPerm.size() > 64 && (int64_t)_byPerm.size() > 2 * _live) {
    size_t kept = 0;
    for (const Back &b : _byPerm) if (Live(b)) _byPerm[kept++] = b;
    _byPerm.resize(kept);
  }
  return true;
}

bool IdLedger::Reissue(int64_t slot) {
  if (!InRange(slot) || _permOf[(size_t)slot] != kNone) return false;   // (a slot that still holds an id is vacated first)
  _permOf[(size_t)slot] = _issueNext;
  Enter(_issueNext++, slot);
  _live++;
  return true;
}

bool IdLedger::Extend(int64_t nSlots) {
  if (nSlots < (int64_t)_permOf.size()) return false;
  _permOf.reserve((size_t)nSlots);
  while ((int64_t)_permOf.size() < nSlots) {
    Enter(_issueNext, (int64_t)_permOf.size());
    _permOf.push_back(_issueNext++);
    _live++;
  }
  return true;
}

// Compaction: the nSlots live slots move to 0 .. nSlots-1, slot i taking the permanent id slot from[i] held.  Checked as a whole
// before anything changes: exactly the live slots, each once.
bool IdLedger::Repack(int64_t nSlots, const int64_t *from) {
  if (nSlots != _live || nSlots > (int64_t)_permOf.size()) return false;
  std::vector<int64_t> packed((size_t)nSlots);
  std::vector<bool> taken(_permOf.size(), false);
  for (int64_t i = 0; i < nSlots; i++) {
    const int64_t src = from[i];
    if (!InRange(src) || _permOf[(size_t)src] == kNone || taken[(size_t)src]) return false;
    taken[(size_t)src] = true;
    packed[(size_t)i] = _permOf[(size_t)src];
  }
  _permOf.swap(packed);
  Rebuild();
  return true;
}

bool IdLedger::Rename(int64_t permanent, int64_t toPermanent) {
  if (toPermanent < 0 || toPermanent >= _issueNext) return false;   // only ids that can no longer be issued (the reference lets the
                                                                    // invalid id -1 through and corrupts its maps with it: refused here)
  if (SlotOf(toPermanent) != kNone) return false;       // in use
  const int64_t slot = SlotOf(permanent);
  if (slot == kNone) return false;
  _permOf[(size_t)slot] = toPermanent;                  // the old id's entry becomes a leftover
  Enter(toPermanent, slot);
  return true;
}

std::vector<int64_t> QuizzesToLetGo(const std::vector<QuizUsage> &quizzes, time_t now, int64_t maxCount, double maxAgeSec) {
  std::vector<int64_t> out;
  std::vector<QuizUsage> rest;
  for (const QuizUsage &u : quizzes) {
    if (difftime(now, u.lastUsage) > maxAgeSec) out.push_back(u.id); else rest.push_back(u);
  }
  if ((int64_t)rest.size() > maxCount) {
    const size_t surplus = rest.size() - (size_t)maxCount;
    // (stable: equal usage times -- the clock has one-second resolution -- stay in registry order)
    std::stable_sort(rest.begin(), rest.end(), [](const QuizUsage &x, const QuizUsage &y) { return x.lastUsage < y.lastUsage; });
    for (size_t i = 0; i < surplus; i++) out.push_back(rest[i].id);
  }
  return out;
}

// ------------------------------------------------------------------------------------------------------------------
// id maps and the quiz registry (reference PqaCore/BaseEngine.cpp:150-215, 780-802)
// ------------------------------------------------------------------------------------------------------------------
bool HipEngine::MapIds(int which, bool toPerm, int64_t count, int64_t *pIds) {
  std::lock_guard<EngineMutex> lk(_mu);
  StopServer();
  // (a shard's question map is the whole axis': GLOBAL compact ids, the same answers on every rank)
  IdLedger &ids = which == 0 ? (IsShard() ? _globalQuestionIds : _questionIds) : which == 1 ? _targetIds : _quizIds;
  for (int64_t i = 0; i < count; i++) pIds[i] = toPerm ? ids.PermanentOf(pIds[i]) : ids.SlotOf(pIds[i]);
  return true;
}
bool HipEngine::EnsurePermQuizGreater(int64_t bound) {
  std::lock_guard<EngineMutex> lk(_mu);
  StopServer();
  return _quizIds.RaiseFloor(bound);
}
bool HipEngine::RemapQuizPermId(int64_t srcPermId, int64_t destPermId) {
  std::lock_guard<EngineMutex> lk(_mu);
  StopServer();
  return _quizIds.Rename(srcPermId, destPermId);
}

int64_t HipEngine::AssignQuiz(Quiz *q) {
  int64_t id;
  if (!_quizGaps.empty()) {
    id = _quizGaps.back();
    _quizGaps.pop_back();
    _quizIds.Reissue(id);
  } else {
    id = (int64_t)_quizzes.size();
    _quizzes.push_back(nullptr);
    _quizIds.Extend((int64_t)_quizzes.size());
  }
  _quizzes[(size_t)id] = q;
  return id;
}

void HipEngine::UnassignQuiz(int64_t iQuiz) {
  _quizzes[(size_t)iQuiz] = nullptr;
  _quizGaps.push_back(iQuiz);
  _quizIds.Vacate(iQuiz);
}

Error HipEngine::ClearOldQuizzes(int64_t maxCount, double maxAgeSec) {  // behaviour: BaseEngine.cpp:814-873
  if (maxCount < 0)
    return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(maxCount),
                        "The number of quizzes to keep cannot be less than 0.");
  std::lock_guard<EngineMutex> lk(_mu);
  StopServer();
  if (_mode != Mode::Regular) return Error();  // quizzes are not expected to exist in maintenance / shutdown mode
  hipSetDevice(_device);
  hipStreamSynchronize(_stream);
  std::vector<QuizUsage> inUse;
  for (size_t slot = 0; slot < _quizzes.size(); slot++)
    if (_quizzes[slot]) inUse.push_back(QuizUsage{(int64_t)slot, _quizzes[slot]->lastUsage});
  for (int64_t id : QuizzesToLetGo(inUse, time(nullptr), maxCount, maxAgeSec)) {
    Quiz *q = _quizzes[(size_t)id];
    UnassignQuiz(id);
    DestroyQuiz(q);
  }
  return Error();
}

// ------------------------------------------------------------------------------------------------------------------
// the arrays of a .kb file, this engine's questions only: sequential I/O at the file's current position through a bounded
// host staging buffer.  The same code serves a whole-cube engine and every shard of a sharded one (the file orders its rows
// by question, so the shards' blocks follow each other).
// ------------------------------------------------------------------------------------------------------------------
// Two pinned staging buffers in turn: the file's read of one batch runs while the other batch's rows are on their way to the
// device (and a save's write while the next batch comes back), so a large knowledge base moves at the slower of the two rates, not
// at their sum (reference: PqaCore/BaseEngine.cpp:323-385 writes row by row; PqaCore/CudaPersistence.cpp:15-43 stages through one
// pageable buffer).  The mD rows of a batch are ONE strided copy (a row per question, (K + 1) ldT elements apart); a question's K sA
// rows are one.
// fileElem (0: the engine's): bytes of the FILE's number type.  Where it is the engine's, a batch is copied straight between the pinned buffer
// and the cube, as it always was.  Where it differs, the batch passes through a dense block on the device -- pinned buffer -> dense block ->
// convert_rows_kernel -> cube, a save the other way round -- one dense block per pinned buffer, everything in the engine's stream, so the
// overlap of file and bus is the same.  Values that do not fit fp32 are counted on the device and fail the call behind its last batch.
Error HipEngine::IoRows(FILE *f, const char *filePath, bool mD, bool write, int fileElem) {   // sA rows [q][a] of T elements, or mD rows [q]
  hipSetDevice(_device);
  const int fe = fileElem ? fileElem : _elem;
  const bool convert = fe != _elem;
  const size_t rowB = (size_t)_T * (size_t)fe, ldB = (size_t)_ldT * (size_t)_elem;
  const int64_t rowsPerQ = mD ? 1 : _K;
  const int64_t batch = std::max<int64_t>(1, (int64_t)((64u << 20) / (rowB * (size_t)rowsPerQ)));
  const size_t bufBytes = (size_t)std::min(batch, _Q) * (size_t)rowsPerQ * rowB;
  struct Staging {
    char *buf[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    bool pinned = false;
    std::vector<char> pageable[2];
    hipStream_t stream = nullptr;
    char *dense[2] = {nullptr, nullptr};   // the file's rows on the device, where its number type is not the cube's
    unsigned *overflow = nullptr;
    ~Staging() {
      (void)hipStreamSynchronize(stream);   // (an early return -- a failed read, a failed copy -- leaves copies in flight: not under buffers about to go)
      for (int i = 0; i < 2; i++) {
        if (pinned && buf[i]) hipHostFree(buf[i]);
        if (done[i]) hipEventDestroy(done[i]);
        if (dense[i]) hipFree(dense[i]);
      }
      if (overflow) hipFree(overflow);
    }
  } st;
  const int nBuf = _Q > batch ? 2 : 1;
  st.stream = _stream;
  st.pinned = true;
  for (int i = 0; i < nBuf && st.pinned; i++)
    if (hipHostMalloc((void **)&st.buf[i], bufBytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); st.pinned = false; }
  if (!st.pinned) {   // (no pinned memory to be had: pageable staging, the copies then synchronise by themselves)
    for (int i = 0; i < 2; i++) { if (st.buf[i]) hipHostFree(st.buf[i]); st.buf[i] = nullptr; }
    for (int i = 0; i < nBuf; i++) { st.pageable[i].resize(bufBytes); st.buf[i] = st.pageable[i].data(); }
  }
  for (int i = 0; i < nBuf; i++) HIP_TRY(hipEventCreateWithFlags(&st.done[i], hipEventDisableTiming));
  if (convert) {
    for (int i = 0; i < nBuf; i++) HIP_TRY(hipMalloc((void **)&st.dense[i], bufBytes));
    HIP_TRY(hipMalloc((void **)&st.overflow, sizeof(unsigned)));
    HIP_TRY(hipMemsetAsync(st.overflow, 0, sizeof(unsigned), _stream));
  }
  const char *what = mD ? "the target dimension of _mD weights." : "the target dimension of _sA weights.";
  auto copyBatch = [&](char *host, int which, int64_t q0, int64_t nq) -> hipError_t {
    if (convert) {
      const size_t bytes = (size_t)(nq * rowsPerQ) * rowB;
      ConvertRows c{st.dense[which], CubeAt(q0, 0), fe, _elem, _T, _ldT, nq * rowsPerQ, rowsPerQ, mD ? _K : 0, _K + 1, !write, false, st.overflow};
      if (write) {
        const hipError_t he = LaunchConvertRows(c, _stream);
        return he != hipSuccess ? he : hipMemcpyAsync(host, st.dense[which], bytes, hipMemcpyDeviceToHost, _stream);
      }
      const hipError_t he = hipMemcpyAsync(st.dense[which], host, bytes, hipMemcpyHostToDevice, _stream);
      return he != hipSuccess ? he : LaunchConvertRows(c, _stream);
    }
    if (mD) {   // one row per question, (K + 1) ldT elements apart
      return write ? hipMemcpy2DAsync(host, rowB, CubeAt(q0, _K), ldB * (size_t)(_K + 1), rowB, (size_t)nq, hipMemcpyDeviceToHost, _stream)
                   : hipMemcpy2DAsync(CubeAt(q0, _K), ldB * (size_t)(_K + 1), host, rowB, rowB, (size_t)nq, hipMemcpyHostToDevice, _stream);
    }
    for (int64_t q = 0; q < nq; q++) {
      char *h = host + (size_t)q * (size_t)rowsPerQ * rowB;
      char *d = CubeAt(q0 + q, 0);
      const hipError_t he = write ? hipMemcpy2DAsync(h, rowB, d, ldB, rowB, (size_t)rowsPerQ, hipMemcpyDeviceToHost, _stream)
                                  : hipMemcpy2DAsync(d, ldB, h, rowB, rowB, (size_t)rowsPerQ, hipMemcpyHostToDevice, _stream);
      if (he != hipSuccess) return he;
    }
    return hipSuccess;
  };
  int64_t prevQ0 = -1, prevNq = 0;   // a save: the batch whose rows are on their way into the other buffer
  int turn = 0;
  for (int64_t q0 = 0; q0 < _Q; q0 += batch, turn ^= (nBuf - 1)) {
    const int64_t nq = std::min(batch, _Q - q0);
    const size_t nRows = (size_t)(nq * rowsPerQ);
    char *host = st.buf[turn];
    HIP_TRY(hipEventSynchronize(st.done[turn]));   // (whatever used this buffer two batches ago has finished; a fresh event is complete)
    if (!write) {
      if (std::fread(host, rowB, nRows, f) != nRows) { (void)hipStreamSynchronize(_stream); return FileErr(filePath, (std::string("Can't read ") + what).c_str()); }
      HIP_TRY(copyBatch(host, turn, q0, nq));
      HIP_TRY(hipEventRecord(st.done[turn], _stream));
    } else {
      HIP_TRY(copyBatch(host, turn, q0, nq));
      HIP_TRY(hipEventRecord(st.done[turn], _stream));
      if (prevQ0 >= 0) {   // while this batch comes back, the previous one goes to the file
        const int other = turn ^ (nBuf - 1);
        HIP_TRY(hipEventSynchronize(st.done[other]));
        if (std::fwrite(st.buf[other], rowB, (size_t)(prevNq * rowsPerQ), f) != (size_t)(prevNq * rowsPerQ)) { (void)hipStreamSynchronize(_stream); return FileErr(filePath, (std::string("Can't write ") + what).c_str()); }
      }
      if (nBuf == 1) {   // (a single batch: written right away)
        HIP_TRY(hipEventSynchronize(st.done[turn]));
        if (std::fwrite(host, rowB, nRows, f) != nRows) return FileErr(filePath, (std::string("Can't write ") + what).c_str());
      } else { prevQ0 = q0; prevNq = nq; }
    }
  }
  HIP_TRY(hipStreamSynchronize(_stream));
  if (write && nBuf == 2 && prevQ0 >= 0) {   // the last batch of a save
    const int last = turn ^ 1;
    if (std::fwrite(st.buf[last], rowB, (size_t)(prevNq * rowsPerQ), f) != (size_t)(prevNq * rowsPerQ)) return FileErr(filePath, (std::string("Can't write ") + what).c_str());
  }
  if (convert) {
    unsigned lost = 0;
    HIP_TRY(hipMemcpy(&lost, st.overflow, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (lost != 0) return KbOverflowErr(filePath, mD ? "_mD" : "_sA", lost);
  }
  return Error();
}

// ... of an array of a .kb file do not fit TPqaPrecisionType::Float: the load (or the save) that asked for it fails
Error KbOverflowErr(const char *filePath, const char *array, uint64_t count) {
  return Error::MakeP(ErrCode::FileOp, std::string("filePath=[") + filePath + "] array=" + array + " values=" + std::to_string(count),
                      std::string("Finite values of the ") + array + " weights overflow TPqaPrecisionType::Float.");
}

// vB: fp64 on the device in both precisions, the words holding the engine's number type; the file holds ITS number type.  Where that
// is the engine's, the conversion is the host's, as it was.  Where it differs, the vector passes through the kernel of the rows: a
// Double file into a Float engine rounds every word through fp32 (and counts what does not fit), a Float file widens, a Double
// engine's save as Float rounds; a Float engine's words ARE the doubles a Double file holds.
Error HipEngine::IoVB(FILE *f, const char *filePath, bool write, int fileElem) {
  hipSetDevice(_device);
  const int fe = fileElem ? fileElem : _elem;
  std::vector<double> vb((size_t)_T);
  std::vector<float> vf(fe == 4 ? (size_t)_T : 0);
  if (fe != _elem) {
    const size_t bytes = (size_t)_T * (size_t)fe;
    void *host = fe == 8 ? (void *)vb.data() : (void *)vf.data();
    struct Dev { char *dense = nullptr; unsigned *overflow = nullptr; ~Dev() { hipFree(dense); hipFree(overflow); } } d;
    HIP_TRY(hipMalloc((void **)&d.dense, bytes));
    HIP_TRY(hipMalloc((void **)&d.overflow, sizeof(unsigned)));
    HIP_TRY(hipMemsetAsync(d.overflow, 0, sizeof(unsigned), _stream));
    ConvertRows c{d.dense, _dVB, fe, 8, _T, _ldT, 1, 1, 0, 0, !write, !write && fe == 8, d.overflow};
    if (write) {
      if (fe == 8) HIP_TRY(hipMemcpyAsync(host, _dVB, bytes, hipMemcpyDeviceToHost, _stream));
      else {
        HIP_TRY(LaunchConvertRows(c, _stream));
        HIP_TRY(hipMemcpyAsync(host, d.dense, bytes, hipMemcpyDeviceToHost, _stream));
      }
    } else {
      if (std::fread(host, (size_t)fe, (size_t)_T, f) != (size_t)_T) return FileErr(filePath, "Can't read the _vB weights.");
      HIP_TRY(hipMemcpyAsync(d.dense, host, bytes, hipMemcpyHostToDevice, _stream));
      HIP_TRY(LaunchConvertRows(c, _stream));
    }
    unsigned lost = 0;
    HIP_TRY(hipMemcpyAsync(&lost, d.overflow, sizeof(unsigned), hipMemcpyDeviceToHost, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
    if (lost != 0) return KbOverflowErr(filePath, "_vB", lost);
    if (write && std::fwrite(host, (size_t)fe, (size_t)_T, f) != (size_t)_T) return FileErr(filePath, "Can't write the _vB weights.");
    return Error();
  }
  if (write) {
    HIP_TRY(hipMemcpyAsync(vb.data(), _dVB, (size_t)_T * sizeof(double), hipMemcpyDeviceToHost, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
    bool ok;
    if (_elem == 8) ok = std::fwrite(vb.data(), sizeof(double), (size_t)_T, f) == (size_t)_T;
    else {
      std::copy(vb.begin(), vb.end(), vf.begin());
      ok = std::fwrite(vf.data(), sizeof(float), (size_t)_T, f) == (size_t)_T;
    }
    return ok ? Error() : FileErr(filePath, "Can't write the _vB weights.");
  }
  if (_elem == 8) {
    if (std::fread(vb.data(), sizeof(double), (size_t)_T, f) != (size_t)_T) return FileErr(filePath, "Can't read the _vB weights.");
  } else {
    if (std::fread(vf.data(), sizeof(float), (size_t)_T, f) != (size_t)_T) return FileErr(filePath, "Can't read the _vB weights.");
    std::copy(vf.begin(), vf.end(), vb.begin());
  }
  return SetVBFromHost(vb.data());
}

Error HipEngine::SetVBFromHost(const double *vb) {
  hipSetDevice(_device);
  HIP_TRY(hipMemcpyAsync(_dVB, vb, (size_t)_T * sizeof(double), hipMemcpyHostToDevice, _stream));
  HIP_TRY(hipStreamSynchronize(_stream));
  return Error();
}

// ------------------------------------------------------------------------------------------------------------------
// .kb persistence (layout of reference PqaCore/BaseEngine.cpp:323-385 + PqaCore/CpuEngine.cpp:664-688):
//   PrecisionDefinition (8 B) | EngineDimensions {nAnswers, nQuestions, nTargets} | u64 nQuestionsAsked |
//   sA rows [q][a] of nTargets doubles | mD rows [q] | vB | question gaps (i64 n, n ids) | target gaps |
//   PermanentIdManager x3 (questions, targets, quizzes saved empty)
// ------------------------------------------------------------------------------------------------------------------
// PrecisionDefinition bitfield of reference PqaCore/Interface/PqaCommon.h:26-32 (type:4, mantissa:28, exponent:16, reserved:16)
uint64_t PackPrecision(uint64_t type, uint64_t mantissa, uint64_t exponent) {
  return (type & 0xF) | ((mantissa & 0xFFFFFFF) << 4) | ((exponent & 0xFFFF) << 32);
}
CiEngineDefinition KbHeader::Definition() const {
  CiEngineDefinition def;
  std::memset(&def, 0, sizeof(def));
  def._nAnswers = K; def._nQuestions = Q; def._nTargets = T;
  def._precType = (uint8_t)(precision & 0xF);
  def._precMantissa = (uint32_t)((precision >> 4) & 0xFFFFFFF);
  def._precExponent = (uint16_t)((precision >> 32) & 0xFFFF);
  def._initAmount = 1.0;
  return def;
}

KbFile::KbFile(const char *filePath, bool write) : path(filePath) {
  if (!path) opened = Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of KB file name.");
  else if (!(f = std::fopen(path, write ? "wb" : "rb")))
    opened = Error::MakeP(ErrCode::CantOpenFile, std::string("filePath=[") + path + "]", write ? "Can't open the file to write KB to." : "Can't open the KB file to read.");
}
Error KbFile::WriteHeader(const KbHeader &h) {
  if (!f) return opened;
  if (std::fwrite(&h.precision, 8, 1, f) != 1) return FileErr(path, "Can't write precision definition header.");   // Double | Float: the element type of the arrays
  if (std::fwrite(&h.K, 8, 3, f) != 3) return FileErr(path, "Can't write engine dimensions header.");
  if (std::fwrite(&h.nAsked, 8, 1, f) != 1) return FileErr(path, "Can't write the number of questions asked.");
  return Error();
}
Error KbFile::ReadHeader(KbHeader &h) {
  if (!f) return opened;
  if (std::fread(&h.precision, 8, 1, f) != 1) return FileErr(path, "Can't read precision definition header.");
  if (std::fread(&h.K, 8, 3, f) != 3) return FileErr(path, "Can't read engine dimensions header.");
  if (std::fread(&h.nAsked, 8, 1, f) != 1) return FileErr(path, "Can't read the number of questions asked.");
  return Error();
}

static bool WriteGaps(FILE *f, const std::vector<int64_t> &gaps) {   // (LIFO order, as the reference's GapTracker saves it)
  const int64_t n = (int64_t)gaps.size();
  return std::fwrite(&n, 8, 1, f) == 1 && std::fwrite(gaps.data(), 8, (size_t)n, f) == (size_t)n;
}
static bool ReadGaps(FILE *f, std::vector<int64_t> &gaps, int64_t limit) {
  int64_t n;
  if (std::fread(&n, 8, 1, f) != 1 || n < 0 || n > limit) return false;
  gaps.resize((size_t)n);
  if (std::fread(gaps.data(), 8, (size_t)n, f) != (size_t)n) return false;
  for (int64_t g : gaps) if (g < 0 || g >= limit) return false;
  return true;
}

// (the live quiz map is written without its slots and keeps its next permanent id, as BaseEngine.cpp:379 writes it)
Error KbFile::WriteTrailer(const std::vector<int64_t> &qGaps, const std::vector<int64_t> &tGaps, const IdLedger &questionIds,
                           const IdLedger &targetIds, const IdLedger &quizIds) {
  if (!WriteGaps(f, qGaps)) return FileErr(path, "Can't write the question gaps.");
  if (!WriteGaps(f, tGaps)) return FileErr(path, "Can't write the target gaps.");
  if (!questionIds.Write(f)) return FileErr(path, "Can't write the question permanent-compact ID mappings.");
  if (!targetIds.Write(f)) return FileErr(path, "Can't write the target permanent-compact ID mappings.");
  if (!quizIds.Write(f, true)) return FileErr(path, "Can't write the quiz permanent-compact ID mappings.");
  return Error();
}
Error KbFile::ReadTrailer(int64_t Q, int64_t T, std::vector<int64_t> &qGaps, std::vector<int64_t> &tGaps, IdLedger &questionIds,
                          IdLedger &targetIds, IdLedger &quizIds) {
  if (!ReadGaps(f, qGaps, Q)) return FileErr(path, "Can't read the question gaps.");
  if (!ReadGaps(f, tGaps, T)) return FileErr(path, "Can't read the target gaps.");
  if (!questionIds.Read(f)) return FileErr(path, "Can't read the question permanent-compact ID mapping.");
  if (!targetIds.Read(f)) return FileErr(path, "Can't read the target permanent-compact ID mapping.");
  if (!quizIds.Read(f)) return FileErr(path, "Can't read the quizzes permanent-compact ID mapping.");
  return Error();
}
Error KbFile::FlushAndClose() {
  if (std::fflush(f) != 0) return FileErr(path, "Failed in hard flushing the KB.");
  FILE *open = f;
  f = nullptr;
  if (std::fclose(open) != 0) return FileErr(path, "Failed in closing the file.");
  return Error();
}

// The header a file of `precType` (0: the engine's own) carries when this engine writes it: the engine's own definition where the
// type is its own -- the bytes SaveKB writes --, otherwise what an engine created in that type writes (the IEEE widths).
Error KbSavePrecision(uint8_t precType, uint8_t ownType, uint32_t ownMantissa, uint16_t ownExponent, uint64_t &packed, int &fileElem) {
  if (precType == 0) precType = ownType;
  if (precType != 1 && precType != 3)
    return Error::MakeP(ErrCode::NotImplemented, "Feature=precType " + std::to_string((int)precType), "A .kb file is written as TPqaPrecisionType::Float or ::Double.");
  fileElem = precType == 1 ? 4 : 8;
  packed = precType == ownType ? PackPrecision(ownType, ownMantissa, ownExponent) : precType == 1 ? PackPrecision(1, 24, 8) : PackPrecision(3, 53, 11);
  return Error();
}

// What a header must say before anything is allocated for it: a number type the engines have, the reference's minimum dimensions
// (PqaEngineBaseFactory.cpp:29-42), and arrays that fit the file -- a damaged header's dimensions come back as an error, not as an
// allocation.
Error KbFile::CheckHeader(const KbHeader &h, KbLayout &layout) const {
  const uint64_t type = h.precision & 0xF;
  if (type != 1 && type != 3)
    return Error::MakeP(ErrCode::NotImplemented, std::string("filePath=[") + path + "] precType=" + std::to_string(type),
                        "The KB file's precision is neither TPqaPrecisionType::Float nor ::Double.");
  layout = KbLayout(h.K, h.Q, h.T, type == 1 ? 4 : 8);
  if (h.K < 2 || h.Q < 1 || h.T < 2 || !layout.valid)
    return Error::MakeP(ErrCode::FileOp, std::string("filePath=[") + path + "] nAnswers=" + std::to_string(h.K) + " nQuestions=" + std::to_string(h.Q) +
                        " nTargets=" + std::to_string(h.T), "The KB file's header does not hold the dimensions of a knowledge base.");
  const int64_t size = Size();
  if (size < layout.ArraysEnd())
    return Error::MakeP(ErrCode::FileOp, std::string("filePath=[") + path + "] size=" + std::to_string(size) + " arrays=" + std::to_string(layout.ArraysEnd()),
                        "The KB file is shorter than the arrays its header announces.");
  return Error();
}
int64_t KbFile::Size() const {
  struct stat st;
  return f && fstat(fileno(f), &st) == 0 ? (int64_t)st.st_size : -1;
}
Error KbFile::Seek(int64_t offset) {
  return fseeko(f, (off_t)offset, SEEK_SET) == 0 ? Error() : FileErr(path, "Can't seek in the KB file.");
}
// in place: the file is opened for writing without being emptied (created where there is none) -- a shard's part of a save
KbFile::KbFile(const char *filePath, InPlace) : path(filePath) {
  if (!path) { opened = Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of KB file name."); return; }
  const int fd = ::open(path, O_RDWR | O_CREAT, 0666);
  if (fd < 0 || !(f = fdopen(fd, "r+b"))) {
    if (fd >= 0) ::close(fd);
    opened = Error::MakeP(ErrCode::CantOpenFile, std::string("filePath=[") + path + "]", "Can't open the file to write KB to.");
  }
}

Error HipEngine::SaveKB(const char *filePath, bool doubleBuffer) {
  (void)doubleBuffer;  // the device copy already is the "second buffer": the file is written from a host snapshot
  return SaveKBAs(filePath, 0);
}

Error HipEngine::SaveKBAs(const char *filePath, uint8_t precType) {
  std::lock_guard<EngineMutex> lk(_mu);
  StopServer();
  if (_qTotal != _Q) return Error::MakeP(ErrCode::NotImplemented, "Feature=SaveKB of a sharded engine", "Save the shards' owner instead.");
  uint64_t precision = 0;
  int fe = 0;
  Error e = KbSavePrecision(precType, _precType, _precMantissa, _precExponent, precision, fe);
  if (!e.ok()) return e;
  KbFile file(filePath, true);
  hipSetDevice(_device);
  e = file.WriteHeader(KbHeader{precision, _K, _Q, _T, _nQuestionsAsked.load(std::memory_order_acquire)});
  if (e.ok()) e = IoRows(file.f, filePath, false, true, fe);   // sA rows [q][a]
  if (e.ok()) e = IoRows(file.f, filePath, true, true, fe);    // mD rows [q]
  if (e.ok()) e = IoVB(file.f, filePath, true, fe);
  if (e.ok()) e = file.WriteTrailer(_questionGapList, _targetGapList, _questionIds, _targetIds, _quizIds);
  return e.ok() ? file.FlushAndClose() : e;
}

// A shard's part of a save, in place: its sA block and its mD block at their offsets of a file that is not emptied first; the shard
// that holds question 0 also writes the header (with its own count of questions asked: every rank sees every Train), vB and the
// trailer, and cuts the file behind the trailer.  The file is complete once every shard's call has returned, in any order.  A whole
// engine is the one shard of its file: the call then writes what SaveKBAs writes.
Error HipEngine::SaveKBShard(const char *filePath, uint8_t precType) {
  std::lock_guard<EngineMutex> lk(_mu);
  StopServer();
  uint64_t precision = 0;
  int fe = 0;
  Error e = KbSavePrecision(precType, _precType, _precMantissa, _precExponent, precision, fe);
  if (!e.ok()) return e;
  const KbLayout lay(_K, _qTotal, _T, fe);
  if (!lay.HasWindow(_qFirst, _Q)) return Error::Make(ErrCode::Internal, "SaveKBShard: the shard's range does not fit its file.");
  KbFile file(filePath, KbFile::InPlace{});
  if (!file.f) return file.opened;
  hipSetDevice(_device);
  e = file.Seek(lay.SaOffset(_qFirst));
  if (e.ok()) e = IoRows(file.f, filePath, false, true, fe);
  if (e.ok()) e = file.Seek(lay.MdOffset(_qFirst));
  if (e.ok()) e = IoRows(file.f, filePath, true, true, fe);
  if (e.ok() && _qFirst == 0) {
    e = file.Seek(0);
    if (e.ok()) e = file.WriteHeader(KbHeader{precision, _K, _qTotal, _T, _nQuestionsAsked.load(std::memory_order_acquire)});
    if (e.ok()) e = file.Seek(lay.vbOff);
    if (e.ok()) e = IoVB(file.f, filePath, true, fe);
    if (e.ok())   // (a shard: the whole question axis as every rank keeps it)
      e = IsShard() ? file.WriteTrailer(_globalQuestionGaps, _targetGapList, _globalQuestionIds, _targetIds, _quizIds)
                    : file.WriteTrailer(_questionGapList, _targetGapList, _questionIds, _targetIds, _quizIds);
    if (e.ok() && (std::fflush(file.f) != 0 || ftruncate(fileno(file.f), ftello(file.f)) != 0)) e = FileErr(filePath, "Can't cut the KB file behind its trailer.");
  }
  return e.ok() ? file.FlushAndClose() : e;
}

HipEngine *HipEngine::Load(Error &err, const char *filePath) {  // PqaEngineBaseFactory.cpp:44-83, CpuEngine.cpp:41-92
  return LoadAs(err, filePath, 0, nullptr, 0);
}

// The engine definition a file is loaded under: the file's own, or -- precType given and not the file's -- that type with the widths
// an engine created in it carries.
Error KbLoadDefinition(const KbHeader &h, uint8_t precType, CiEngineDefinition &def) {
  def = h.Definition();
  if (precType == 0 || precType == def._precType) return Error();
  if (precType != 1 && precType != 3)
    return Error::MakeP(ErrCode::NotImplemented, "Feature=precType " + std::to_string((int)precType), "A .kb file is loaded as TPqaPrecisionType::Float or ::Double.");
  def._precType = precType;
  def._precMantissa = precType == 1 ? 24 : 53;
  def._precExponent = precType == 1 ? 8 : 11;
  return Error();
}

// Load in the file's precision or another (precType), whole (shard == nullptr) or the window [shard->_qFirst, + nLocal) of the
// file's questions as a shard on shard->_device.  A shard takes its rows -- a seek to each of its two blocks --, the whole vB, the
// target gaps, the target and quiz ledgers, and the question gaps of its range as local gap bits; the file's question gap list and
// question id ledger become its view of the whole question axis (_globalQuestionGaps, _globalQuestionIds).
HipEngine *HipEngine::LoadAs(Error &err, const char *filePath, uint8_t precType, const CiHipShard *shard, int64_t nLocal) {
  KbFile file(filePath, false);
  KbHeader h;
  err = file.ReadHeader(h);
  if (!err.ok()) return nullptr;
  KbLayout lay;
  err = file.CheckHeader(h, lay);
  if (!err.ok()) return nullptr;
  CiEngineDefinition def;
  err = KbLoadDefinition(h, precType, def);
  if (!err.ok()) return nullptr;
  CiHipShard window{0, h.Q, -1, 0};
  if (shard) {
    if (nLocal < 0) { err = Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(nLocal), "The number of local questions cannot be negative."); return nullptr; }
    if (shard->_qTotal != 0 && shard->_qTotal != h.Q) {
      err = Error::MakeP(ErrCode::InsufficientEngineDimensions, "[_qTotal=" + std::to_string(shard->_qTotal) + " of " + std::to_string(h.Q) + "]",
                         "The shard's total question count is not the KB file's.");
      return nullptr;
    }
    if (!lay.HasWindow(shard->_qFirst, nLocal)) {
      err = Error::MakeP(ErrCode::IndexOutOfRange, "[" + std::to_string(shard->_qFirst) + ", " + std::to_string(shard->_qFirst) + " + " + std::to_string(nLocal) + ") of " +
                         std::to_string(h.Q), "The shard's question range is not within the KB file's.");
      return nullptr;
    }
    window._qFirst = shard->_qFirst;
    window._device = shard->_device;
    def._nQuestions = nLocal;
  }
  std::unique_ptr<HipEngine> eng(HipEngine::Create(err, def, shard ? &window : nullptr));
  if (!eng) return nullptr;
  HipEngine &e = *eng;
  hipSetDevice(e._device);
  const int fe = (int)lay.elem;
  err = file.Seek(lay.SaOffset(e._qFirst));
  if (err.ok()) err = e.IoRows(file.f, filePath, false, false, fe);
  if (err.ok()) err = file.Seek(lay.MdOffset(e._qFirst));
  if (err.ok()) err = e.IoRows(file.f, filePath, true, false, fe);
  if (err.ok()) err = file.Seek(lay.vbOff);
  if (err.ok()) err = e.IoVB(file.f, filePath, false, fe);
  if (!err.ok()) return nullptr;
  e._nQuestionsAsked.store(h.nAsked);
  if (e._qTotal == e._Q) {
    err = file.ReadTrailer(e._Q, e._T, e._questionGapList, e._targetGapList, e._questionIds, e._targetIds, e._quizIds);
    if (!err.ok()) return nullptr;
    for (int64_t g : e._questionGapList) BitSet(e._hQGap, g, true);
  } else {
    err = file.ReadTrailer(h.Q, e._T, e._globalQuestionGaps, e._targetGapList, e._globalQuestionIds, e._targetIds, e._quizIds);
    if (!err.ok()) return nullptr;
    for (int64_t g : e._globalQuestionGaps)
      if (e.OwnsQuestion(g) && !BitTest(e._hQGap, g - e._qFirst)) {
        BitSet(e._hQGap, g - e._qFirst, true);
        e._questionGapList.push_back(g - e._qFirst);
        e._questionIds.Vacate(g - e._qFirst);
      }
  }
  for (int64_t g : e._targetGapList) BitSet(e._hTGap, g, true);
  e._nTargetGaps = (int64_t)e._targetGapList.size();
  err = e.UploadGaps();
  return err.ok() ? eng.release() : nullptr;
}

Error CheckAddArgs(int64_t nQuestions, const CiAddQorTParam *pAqps, int64_t nTargets, const CiAddQorTParam *pAtps) {
  if (nQuestions < 0 || nTargets < 0)
    return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(std::min(nQuestions, nTargets)), "Counts must be non-negative.");
  if ((nQuestions > 0 && !pAqps) || (nTargets > 0 && !pAtps)) return Error::Make(ErrCode::NullArgument, "Nullptr parameters array.");
  return Error();
}
Error WrongModeErr(const char *what) {
  return Error::Make(ErrCode::WrongMode, std::string("Can't perform maintenance-only mode operation - ") + what +
                                             " - because current mode is not maintenance (but regular/shutdown?).");
}

// ------------------------------------------------------------------------------------------------------------------
// maintenance-mode operations
// ------------------------------------------------------------------------------------------------------------------
namespace {
// device allocation that is freed unless released: every buffer of a resize exists before the first one is committed
template <typename T>
struct DevBuf {
  T *p = nullptr;
  ~DevBuf() { if (p) hipFree(p); }
  hipError_t Alloc(size_t bytes) { return hipMalloc(reinterpret_cast<void **>(&p), bytes); }
  T *Release() { T *r = p; p = nullptr; return r; }
};
}  // namespace

// Grow the knowledge base to newQ questions and newT targets.  All-or-nothing: every new buffer is allocated and filled
// before the engine's members change, so a failure (out of memory while the old and the new cube coexist) leaves the engine
// as it was.
Error HipEngine::ReallocKB(int64_t newQ, int64_t newT, int64_t newQTotal) {
  const int64_t newLdT = std::max(_ldT, RoundLdT(newT, _elem));
  const int64_t newCap = std::max(_capQ, newQ);
  const bool regrow = newLdT != _ldT || newCap != _capQ;
  DevBuf<char> cube;
  DevBuf<double> vB, priority, runLength, poleScratch;
  DevBuf<int64_t> exps;
  DevBuf<uint32_t> tgapDev, qgapDev;
  // bitmaps: keep the old bits, new positions are not gaps, everything past the size is
  std::vector<uint32_t> tg(BitWords(newLdT), 0), qg(BitWords(newQ), 0);
  for (int64_t t = 0; t < _T; t++) if (BitTest(_hTGap, t)) BitSet(tg, t, true);
  for (int64_t t = newT; t < (int64_t)tg.size() * 32; t++) BitSet(tg, t, true);
  for (int64_t q = 0; q < _Q; q++) if (BitTest(_hQGap, q)) BitSet(qg, q, true);
  for (int64_t q = newQ; q < (int64_t)qg.size() * 32; q++) BitSet(qg, q, true);
  HIP_TRY(tgapDev.Alloc(tg.size() * sizeof(uint32_t)));
  HIP_TRY(qgapDev.Alloc(qg.size() * sizeof(uint32_t)));
  if (regrow) {
    const size_t el = (size_t)_elem;
    HIP_TRY(cube.Alloc((size_t)newCap * (size_t)(_K + 1) * (size_t)newLdT * el));
    HIP_TRY(vB.Alloc((size_t)newLdT * sizeof(double)));
    if (newLdT != _ldT) HIP_TRY(exps.Alloc((size_t)newLdT * sizeof(int64_t)));
    if (newCap != _capQ) {
      HIP_TRY(priority.Alloc((size_t)newCap * sizeof(double)));
      HIP_TRY(runLength.Alloc((size_t)newCap * sizeof(double)));
      HIP_TRY(poleScratch.Alloc(PoleScratchBytes(newCap)));
      HIP_TRY(hipMemsetAsync(poleScratch.p, 0, PoleScratchBytes(newCap), _stream));
    }
    // old rows keep their content; new padding columns get A = 0, D = 1 from the fill of new questions / a plain fill
    HIP_TRY(LaunchFillFresh(cube.p, _elem, vB.p, _K, newCap, 0, newLdT, 0.0, _stream));  // T = 0: every column is "padding"
    HIP_TRY(hipMemcpy2DAsync(cube.p, (size_t)newLdT * el, _dCube, (size_t)_ldT * el, (size_t)_T * el,
                             (size_t)_Q * (size_t)(_K + 1), hipMemcpyDeviceToDevice, _stream));
    HIP_TRY(hipMemcpyAsync(vB.p, _dVB, (size_t)_T * sizeof(double), hipMemcpyDeviceToDevice, _stream));
    HIP_TRY(hipStreamSynchronize(_stream));
  }
  // ---- commit (nothing below can fail except the bitmap upload, which leaves host and device views consistent in shape)
  if (regrow) {
    hipFree(_dCube); hipFree(_dVB);
    _dCube = cube.Release(); _dVB = vB.Release();
    if (exps.p) { hipFree(_dExps); _dExps = exps.Release(); }
    if (priority.p) {
      hipFree(_dPriority); hipFree(_dRunLength); hipFree(_dPoleScratch);
      _dPriority = priority.Release(); _dRunLength = runLength.Release(); _dPoleScratch = poleScratch.Release();
    }
    _ldT = newLdT;
    _capQ = newCap;
  }
  _hTGap.swap(tg);
  _hQGap.swap(qg);
  hipFree(_dTGap); hipFree(_dQGap);
  _dTGap = tgapDev.Release(); _dQGap = qgapDev.Release();
  _Q = newQ;
  _qTotal = newQTotal;
  _T = newT;
  return UploadGaps();
}

// On a shard the call is collective and replicated: every rank plans over the same global gap list and dimensions, so the ids are
// the same everywhere.  Target columns are filled by every shard over its own questions (and its vB replica); a reused question id is
// re-initialised by the shard that holds it; appended ids go to the shard whose range ends at the question count -- its _Q and capacity
// grow --, every other shard only raises _qTotal.  A whole engine is the one shard that holds everything.
Error HipEngine::AddQsTs(int64_t nQuestions, CiAddQorTParam *pAqps, int64_t nTargets, CiAddQorTParam *pAtps) {
  std::lock_guard<EngineMutex> lk(_mu);
  StopServer();
  if (_mode != Mode::Maintenance) return WrongModeErr("add questions/targets");
  Error ae = CheckAddArgs(nQuestions, pAqps, nTargets, pAtps);
  if (!ae.ok()) return ae;
  hipSetDevice(_device);
  // CpuEngine::AddQsTsSpec, reference PqaCore/CpuEngine.cpp:468-575.  The ids are worked out first (kb_plan.h) and committed
  // -- gap lists, permanent ids, bitmaps, the caller's _index fields -- only after the resize and the fills have succeeded.
  const bool shard = IsShard(), holdsEnd = _qFirst + _Q == _qTotal;
  const AddPlan plan = PlanAdd(shard ? _globalQuestionGaps : _questionGapList, _targetGapList, _qTotal, _T, nQuestions, pAqps, nTargets, pAtps);
  const std::vector<int64_t> &qIds = plan.qIds, &tIds = plan.tIds;
  const int64_t nQReuse = plan.nQReuse, nTReuse = plan.nTReuse, nTNew = nTargets - nTReuse, nQOld = _Q;
  const int64_t newLocalQ = _Q + (holdsEnd ? plan.newQ - _qTotal : 0);
  // the call's questions this engine holds, LOCAL ids: the reused ones first
  std::vector<int64_t> qLocal;
  std::vector<double> qLocalInit;
  int64_t nLocalReuse = 0;
  for (int64_t i = 0; i < nQuestions; i++) {
    const bool mine = i < nQReuse ? OwnsQuestion(qIds[(size_t)i]) : holdsEnd;
    if (!mine) continue;
    qLocal.push_back(qIds[(size_t)i] - _qFirst);
    qLocalInit.push_back(plan.qInit[(size_t)i]);
    if (i < nQReuse) nLocalReuse++;
  }
  // whole questions first, then target columns over the questions not (re)initialised just now
  std::vector<uint32_t> skip(BitWords(newLocalQ), 0);
  for (int64_t i = 0; i < nLocalReuse; i++) BitSet(skip, qLocal[(size_t)i], true);    // :558-560 only reused questions are skipped
  DevBuf<int64_t> dQ, dT;
  DevBuf<double> dQi, dTi;
  DevBuf<uint32_t> dSkip;
  HIP_TRY(Upload(&dQ.p, qLocal, _stream));
  HIP_TRY(Upload(&dQi.p, qLocalInit, _stream));
  HIP_TRY(Upload(&dT.p, tIds, _stream));
  HIP_TRY(Upload(&dTi.p, plan.tInit, _stream));
  HIP_TRY(Upload(&dSkip.p, skip, _stream));
  Error e = ReallocKB(newLocalQ, plan.newT, plan.newQ);   // all-or-nothing; the reused ids are still flagged as gaps
  if (!e.ok()) return e;
  // new target columns apply to every old question (:512-527); reused target columns skip reused questions (:553-567).
  // New questions are filled over ALL columns with their own amount (:497-510), so they are filled last.
  hipError_t he = hipSuccess;
  if (nTReuse > 0) he = LaunchFillTargets(_dCube, _elem, _dVB, _K, _ldT, nQOld, dSkip.p, dT.p, dTi.p, nTReuse, _stream);
  if (he == hipSuccess && nTNew > 0) he = LaunchFillTargets(_dCube, _elem, _dVB, _K, _ldT, nQOld, nullptr, dT.p + nTReuse, dTi.p + nTReuse, nTNew, _stream);
  if (he == hipSuccess && !qLocal.empty()) he = LaunchFillQuestions(_dCube, _elem, _K, _T, _ldT, dQ.p, dQi.p, (int64_t)qLocal.size(), _stream);
  if (he == hipSuccess) he = hipStreamSynchronize(_stream);
  if (he != hipSuccess) {   // (a failed launch: the device is gone) keep the id maps the size of the grown KB
    _questionIds.Extend(_Q);
    _targetIds.Extend(_T);
    if (shard) _globalQuestionIds.Extend(_qTotal);
    return HipErr(he, "AddQsTs");
  }
  // ---- commit
  for (int64_t i = 0; i < nLocalReuse; i++) { BitSet(_hQGap, qLocal[(size_t)i], false); _questionIds.Reissue(qLocal[(size_t)i]); }
  for (int64_t i = 0; i < nTReuse; i++) { BitSet(_hTGap, tIds[(size_t)i], false); _targetIds.Reissue(tIds[(size_t)i]); }
  if (shard) {   // the whole axis, and this shard's own list (its order is not the global one's: the reused ids are looked up)
    for (int64_t i = 0; i < nQReuse; i++) _globalQuestionIds.Reissue(qIds[(size_t)i]);
    _globalQuestionGaps.resize(_globalQuestionGaps.size() - (size_t)nQReuse);
    _globalQuestionIds.Extend(_qTotal);
    for (int64_t i = 0; i < nLocalReuse; i++) {
      const auto at = std::find(_questionGapList.begin(), _questionGapList.end(), qLocal[(size_t)i]);
      if (at != _questionGapList.end()) _questionGapList.erase(at);
    }
  } else {
    _questionGapList.resize(_questionGapList.size() - (size_t)nQReuse);   // (the reused ids were its last entries)
  }
  _targetGapList.resize(_targetGapList.size() - (size_t)nTReuse);
  _nTargetGaps = (int64_t)_targetGapList.size();
  _questionIds.Extend(_Q);                           // :541-542
  _targetIds.Extend(_T);
  for (int64_t i = 0; i < nQuestions; i++) pAqps[i]._index = qIds[(size_t)i];
  for (int64_t j = 0; j < nTargets; j++) pAtps[j]._index = tIds[(size_t)j];
  return UploadGaps();
}

Error HipEngine::AdoptRows(const std::vector<const void *> &srcBlocks, int64_t ldTsrc, const std::vector<int64_t> &colMap, const double *srcVB) {
  std::lock_guard<EngineMutex> lk(_mu);
  StopServer();
  if ((int64_t)srcBlocks.size() != _Q || (int64_t)colMap.size() != _T)
    return Error::Make(ErrCode::Internal, "AdoptRows: the maps do not have this shard's dimensions.");
  hipSetDevice(_device);
  const void **dSrc = nullptr;
  int64_t *dMap = nullptr;
  hipError_t he = Upload(&dSrc, srcBlocks, _stream);
  if (he == hipSuccess) he = Upload(&dMap, colMap, _stream);
  if (he == hipSuccess) he = LaunchAdoptRows(_dCube, _elem, _dVB, _K, _Q, _T, _ldT, dSrc, ldTsrc, srcVB, dMap, _stream);
  if (he == hipSuccess) he = hipStreamSynchronize(_stream);
  hipFree(dSrc);
  hipFree(dMap);
  if (he != hipSuccess) return HipErr(he, "AdoptRows");
  return Error();
}

Error HipEngine::ApplyFills(const std::vector<int64_t> &tIds, const std::vector<double> &tInit, const std::vector<int64_t> &qLocalIds,
                            const std::vector<double> &qInit) {
  std::lock_guard<EngineMutex> lk(_mu);
  StopServer();
  hipSetDevice(_device);
  DevBuf<int64_t> dQ, dT;
  DevBuf<double> dQi, dTi;
  HIP_TRY(Upload(&dQ.p, qLocalIds, _stream));
  HIP_TRY(Upload(&dQi.p, qInit, _stream));
  HIP_TRY(Upload(&dT.p, tIds, _stream));
  HIP_TRY(Upload(&dTi.p, tInit, _stream));
  // target columns over every question, then whole questions over every column (the reference skips the re-initialised
  // questions in the first step only because the second overwrites them anyway, CpuEngine.cpp:558-560)
  hipError_t he = LaunchFillTargets(_dCube, _elem, _dVB, _K, _ldT, _Q, nullptr, dT.p, dTi.p, (int64_t)tIds.size(), _stream);
  if (he == hipSuccess) he = LaunchFillQuestions(_dCube, _elem, _K, _T, _ldT, dQ.p, dQi.p, (int64_t)qLocalIds.size(), _stream);
  if (he == hipSuccess) he = hipStreamSynchronize(_stream);
  if (he != hipSuccess) return HipErr(he, "ApplyFills");
  return Error();
}

// RemoveQuestions / RemoveTargets validate every id -- range, gaps, repeats within the call -- before the first one is removed:
// a failing call changes nothing, on the host or on the device.  (The reference removes id by id and stops at the first
// bad one, BaseEngine.cpp:722-765, leaving the earlier ones removed.)
Error HipEngine::RemoveQuestions(int64_t n, const int64_t *pQIds) {  // BaseEngine.cpp:722-743
  std::lock_guard<EngineMutex> lk(_mu);
  StopServer();
  if (_mode != Mode::Maintenance) return WrongModeErr("remove questions");
  if (!IsShard()) return RemoveIds(n, pQIds, _Q, _hQGap, _questionGapList, _questionIds, "Question index is not in KB.");
  // A shard: GLOBAL ids, validated against the whole axis' gaps -- the same verdict on every rank --; every rank lists and retires
  // them, the rank that holds one also flags it.
  std::vector<char> isGap((size_t)_qTotal, 0);
  for (int64_t g : _globalQuestionGaps) isGap[(size_t)g] = 1;
  Error e = CheckRemoval(n, pQIds, _qTotal, [&](int64_t id) { return isGap[(size_t)id] != 0; }, "Question index is not in KB.");
  if (!e.ok()) return e;
  for (int64_t i = 0; i < n; i++) {
    const int64_t id = pQIds[i];
    _globalQuestionGaps.push_back(id);
    _globalQuestionIds.Vacate(id);
    if (!OwnsQuestion(id)) continue;
    BitSet(_hQGap, id - _qFirst, true);
    _questionGapList.push_back(id - _qFirst);
    _questionIds.Vacate(id - _qFirst);
  }
  hipSetDevice(_device);
  return UploadGaps();
}

Error HipEngine::RemoveTargets(int64_t n, const int64_t *pTIds) {  // BaseEngine.cpp:745-765
  std::lock_guard<EngineMutex> lk(_mu);
  StopServer();
  if (_mode != Mode::Maintenance) return WrongModeErr("remove targets");
  Error e = RemoveIds(n, pTIds, _T, _hTGap, _targetGapList, _targetIds, "Target index is not in KB (but rather at a gap).");
  _nTargetGaps = (int64_t)_targetGapList.size();
  return e;
}

Error HipEngine::RemoveIds(int64_t n, const int64_t *ids, int64_t limit, std::vector<uint32_t> &gapBits, std::vector<int64_t> &gapList,
                           IdLedger &ledger, const char *absentMsg) {
  Error e = CheckRemoval(n, ids, limit, [&](int64_t id) { return BitTest(gapBits, id); }, absentMsg);
  if (!e.ok()) return e;
  for (int64_t i = 0; i < n; i++) {
    BitSet(gapBits, ids[i], true);
    gapList.push_back(ids[i]);
    ledger.Vacate(ids[i]);
  }
  hipSetDevice(_device);
  return UploadGaps();
}

Error HipEngine::Compact(int64_t *pnQuestions, const int64_t **ppOldQuestions, int64_t *pnTargets, const int64_t **ppOldTargets) {
  return CompactLocked(false, nullptr, 0, -1, pnQuestions, ppOldQuestions, pnTargets, ppOldTargets);
}
Error HipEngine::CompactFromBlocks(const void *pBlocks, int64_t slotBytes, int64_t emptiedRank, int64_t *pnQuestions, const int64_t **ppOldQuestions,
                                   int64_t *pnTargets, const int64_t **ppOldTargets) {
  return CompactLocked(true, pBlocks, slotBytes, emptiedRank, pnQuestions, ppOldQuestions, pnTargets, ppOldTargets);
}

// What a compaction would do, on the host alone: the new dimensions and the whole-question moves as (dst, src) pairs of GLOBAL ids --
// the same on every rank --, and whether THIS engine's range would be left without a question.
Error HipEngine::CompactPlanOf(int64_t *pnQuestions, int64_t *pnTargets, int64_t *pnMoves, const int64_t **ppMoves, uint8_t *pWouldBeEmpty) {
  if (!pnQuestions || !pnTargets || !pnMoves || !ppMoves || !pWouldBeEmpty) return Error::Make(ErrCode::NullArgument, "Nullptr output.");
  std::lock_guard<EngineMutex> lk(_mu);
  const CompactPlan plan = PlanCompact(IsShard() ? _globalQuestionGaps : _questionGapList, _targetGapList, _qTotal, _T);
  std::vector<int64_t> moves;
  for (const auto &mv : plan.qMoves) { moves.push_back(mv.first); moves.push_back(mv.second); }
  *pnQuestions = (int64_t)plan.oldQ.size();
  *pnTargets = (int64_t)plan.oldT.size();
  *pnMoves = (int64_t)plan.qMoves.size();
  *ppMoves = MallocCopy(moves);
  *pWouldBeEmpty = ClippedQuestions(_qFirst, _Q, *pnQuestions) == 0 ? 1 : 0;
  return Error();
}

// One launch (kb_kernels.hip: copy_question_blocks_kernel) behind one copy of the pointer list, as PackAnswerRows; nothing waits
// for the device.  Slot i takes question pQuestions[i] where this engine holds it: its K + 1 rows, T elements each, zeros behind.
Error HipEngine::PackQuestionBlocks(int64_t n, const int64_t *pQuestions, void *pDst, void *pFlag, uint64_t flagValue) {
  if (n < 0) return Error::MakeP(ErrCode::NegativeCount, "count=" + std::to_string(n), "The number of question blocks must be non-negative.");
  if (n > 0 && (!pQuestions || !pDst)) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the questions or the package.");
  std::lock_guard<EngineMutex> lk(_mu);
  if (_mode != Mode::Maintenance) return WrongModeErr("pack question blocks");
  int64_t m = 0;
  for (int64_t i = 0; i < n; i++) {   // (everything is checked before anything is launched)
    if (pQuestions[i] < 0 || pQuestions[i] >= _qTotal)
      return Error::MakeP(ErrCode::IndexOutOfRange, RangeParams(pQuestions[i], 0, _qTotal - 1), "Question index is not in KB range.");
    m += OwnsQuestion(pQuestions[i]) ? 1 : 0;
  }
  if (m == 0 && pFlag == nullptr) return Error();
  hipSetDevice(_device);
  StopServer();
  static_assert(sizeof(BlockCopy) == 2 * sizeof(int64_t), "the blocks travel in the answered-question buffer");
  const int64_t words = 2 + 2 * m;   // {arrival counter, pad}, then a BlockCopy per block of this engine's
  Error e = EnsurePackList(words);
  if (!e.ok()) return e;
  BlockCopy *blocks = reinterpret_cast<BlockCopy *>(_hPack + 2);
  const size_t slotBytes = (size_t)QuestionBlockSlotBytes();
  for (int64_t i = 0, at = 0; i < n; i++)
    if (OwnsQuestion(pQuestions[i])) blocks[at++] = BlockCopy{CubeAt(pQuestions[i] - _qFirst), static_cast<char *>(pDst) + (size_t)i * slotBytes};
  MarkStreamBusy();
  e = SubmitPackList(words);
  if (!e.ok()) return e;
  HIP_TRY(LaunchCopyQuestionBlocks(reinterpret_cast<const BlockCopy *>(_dAqs + 2), m, _K + 1, _T * _elem / 4, _ldT * _elem, (int64_t)slotBytes / (_K + 1), true,
                                   reinterpret_cast<unsigned *>(_dAqs), static_cast<uint64_t *>(pFlag), flagValue, _stream));
  _packCalls++;
  _packBytes += (uint64_t)m * slotBytes;
  return Error();
}

// CpuEngine::CompactSpec, CpuEngine.cpp:577-658.  On a shard the plan is the global axis' (kb_plan.h) and the shard keeps the part
// of its range below the new question count; every move (dst, src) has src among the dropped ids and dst a gap among the kept ones,
// so the moves are independent of each other: this engine makes those whose dst it holds, from its own cube where it holds src too,
// otherwise from slot i of the package (move i of the plan).  Everything is checked before anything moves.
Error HipEngine::CompactLocked(bool fromBlocks, const void *pBlocks, int64_t slotBytes, int64_t emptiedRank, int64_t *pnQuestions,
                               const int64_t **ppOldQuestions, int64_t *pnTargets, const int64_t **ppOldTargets) {
  std::lock_guard<EngineMutex> lk(_mu);
  StopServer();
  if (_mode != Mode::Maintenance) return WrongModeErr("compact the KB");
  if (!pnQuestions || !ppOldQuestions || !pnTargets || !ppOldTargets) return Error::Make(ErrCode::NullArgument, "Nullptr output.");
  const bool shard = IsShard();
  if (shard && !fromBlocks) return Error::MakeP(ErrCode::NotImplemented, "Feature=Compact on a shard", "Compact on a shard: use PqaEngine_CompactFromBlocks");
  if (pBlocks && slotBytes != QuestionBlockSlotBytes())
    return Error::MakeP(ErrCode::IndexOutOfRange, "[slotBytes=" + std::to_string(slotBytes) + " of " + std::to_string(QuestionBlockSlotBytes()) + "]",
                        "The block package's slot size is not this engine's (PqaHip_QuestionBlockSlotBytes).");
  hipSetDevice(_device);
  const CompactPlan plan = PlanCompact(shard ? _globalQuestionGaps : _questionGapList, _targetGapList, _qTotal, _T);   // the pairing: kb_plan.h
  const int64_t nQ = (int64_t)plan.oldQ.size(), nT = (int64_t)plan.oldT.size();
  const int64_t nLocal = shard ? ClippedQuestions(_qFirst, _Q, nQ) : nQ;
  if (emptiedRank >= 0 || (shard && nLocal == 0))   // (the ranks' vote, or at least this shard's own part of it: the same text on every rank)
    return Error::MakeP(ErrCode::InsufficientEngineDimensions, "[nQuestions=" + std::to_string(nQ) + "]" + (emptiedRank >= 0 ? " [rank=" + std::to_string(emptiedRank) + "]" : ""),
                        "The compaction would leave a shard without a question.");
  std::vector<BlockCopy> foreign;
  for (size_t i = 0; i < plan.qMoves.size(); i++) {
    const int64_t dst = plan.qMoves[i].first, src = plan.qMoves[i].second;
    if (!OwnsQuestion(dst) || OwnsQuestion(src)) continue;
    if (pBlocks == nullptr) return Error::Make(ErrCode::NullArgument, "Nullptr is passed in place of the block package.");
    foreign.push_back(BlockCopy{static_cast<const char *>(pBlocks) + i * (size_t)slotBytes, CubeAt(dst - _qFirst)});
  }
  for (const auto &mv : plan.qMoves)
    if (OwnsQuestion(mv.first) && OwnsQuestion(mv.second))
      HIP_TRY(hipMemcpyAsync(CubeAt(mv.first - _qFirst), CubeAt(mv.second - _qFirst), (size_t)(_K + 1) * (size_t)_ldT * (size_t)_elem, hipMemcpyDeviceToDevice, _stream));
  std::vector<int64_t> moves;   // {src, dst} per target column that moves
  for (int64_t t = 0; t < nT; t++) if (plan.oldT[(size_t)t] != t) { moves.push_back(plan.oldT[(size_t)t]); moves.push_back(t); }
  DevBuf<BlockCopy> dForeign;
  DevBuf<int64_t> dMoves;
  hipError_t he = Upload(&dForeign.p, foreign, _stream);
  if (he == hipSuccess && !foreign.empty())
    he = LaunchCopyQuestionBlocks(dForeign.p, (int64_t)foreign.size(), _K + 1, _T * _elem / 4, slotBytes / (_K + 1), _ldT * _elem, false, nullptr, nullptr, 0, _stream);
  if (he == hipSuccess) he = Upload(&dMoves.p, moves, _stream);
  if (he == hipSuccess) he = LaunchMoveTargets(_dCube, _elem, _dVB, _K, _ldT, nLocal, dMoves.p, (int64_t)moves.size() / 2, _stream);
  if (he == hipSuccess) he = hipStreamSynchronize(_stream);
  if (he != hipSuccess) return HipErr(he, "Compact");
  if (shard) {   // the whole axis; the local map starts over (its permanent ids are nobody's: MapIds answers from the global one)
    _globalQuestionIds.Repack(nQ, plan.oldQ.data());
    _globalQuestionGaps.clear();
    _questionIds.Clear();
    _questionIds.Extend(nLocal);
  } else {
    _questionIds.Repack(nQ, plan.oldQ.data());
  }
  _targetIds.Repack(nT, plan.oldT.data());
  _questionGapList.clear();
  _targetGapList.clear();
  _nTargetGaps = 0;
  // shrink the logical dimensions; the allocation (capacity, ldT) stays, padding is re-flagged as gap
  _hTGap.assign(BitWords(_ldT), 0);
  _hQGap.assign(BitWords(nLocal), 0);
  for (int64_t t = nT; t < (int64_t)_hTGap.size() * 32; t++) BitSet(_hTGap, t, true);
  for (int64_t q = nLocal; q < (int64_t)_hQGap.size() * 32; q++) BitSet(_hQGap, q, true);
  hipFree(_dQGap); _dQGap = nullptr;
  HIP_TRY(hipMalloc(&_dQGap, _hQGap.size() * sizeof(uint32_t)));
  _Q = nLocal; _qTotal = nQ; _T = nT;
  *pnQuestions = nQ; *pnTargets = nT;
  *ppOldQuestions = MallocCopy(plan.oldQ); *ppOldTargets = MallocCopy(plan.oldT);
  return UploadGaps();
}

}  // namespace pqa
