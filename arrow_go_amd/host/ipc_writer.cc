// Record batches resident in HBM → an Arrow IPC stream, compressed on the device — see ipc.h (StreamWriter) and DESIGN.md §3.8.
//
// What ipc.NewWriter / Writer.Write / Close do on the host (arrow/ipc/writer.go:85-260, the record encoder :300-700, the metadata
// builders of metadata.go) with one difference in where the bytes are made: the columns never come down uncompressed.  For one
// Write() — the dictionary batches it needs and the record batch —
//   1. every buffer is normalised INTO one device allocation laid out like an uncompressed body (bitmaps shifted to bit 0 by
//      ah_copy_bitmap over zeroed bytes, offsets re-based by the arithmetic kernel, the referenced data range copied);
//   2. with lz4, ONE ah_lz4_compress_blocks launch compresses all of its 64 KiB pieces, and only the size table comes back;
//   3. the host lays out every message — framing, FlatBuffer metadata, and per buffer the length prefix, frame header, block size
//      words, end mark and padding (lz4_frame_layout.h) — and ONE ah_ipc_pack_body launch puts it together in HBM;
//   4. ONE device-to-host copy appends it to the stream.
// Without compression steps 1, 3 and 4 are the same and the pack moves the plain bytes.
//
// The metadata is written by the small FlatBuffer builder below, back to front like the reference's generated code does it: scalars
// aligned to their size counted from the END of the buffer, whose final length is a multiple of 8, vtables in front of their
// tables — what the verifiers of Arrow C++ and arrow-go check before they read a message.
#include <cstring>

#include "../../include/arrowhip.h"
#include "capi_internal.h"
#include "ipc.h"
#include "lz4_frame_layout.h"

namespace arrowhip {
namespace ipc {
namespace {

Status Invalid(const std::string& m) { return Status::Make(StatusCode::Invalid, "arrow/ipc: " + m); }
Status NotImpl(const std::string& m) { return Status::Make(StatusCode::NotImplemented, "arrow/ipc: " + m); }

// ---- a minimal FlatBuffer builder ---------------------------------------------------------------------------------------------
// Positions are counted from the END of the finished buffer ("used" bytes so far), as in the flatbuffers library: an object's
// position is the value of used() right after it was written.
class FbBuilder {
 public:
  size_t used() const { return used_; }
  void Align(size_t a, size_t extra = 0) {   // after `extra` more bytes the position is a multiple of a
    while ((used_ + extra) % a) PushByte(0);
  }
  template <typename T>
  void Push(T v) {
    Align(sizeof(T));
    uint8_t raw[sizeof(T)];
    std::memcpy(raw, &v, sizeof(T));
    for (size_t i = sizeof(T); i-- > 0;) PushByte(raw[i]);   // little-endian, written back to front
  }
  uint32_t String(const std::string& s) {
    Align(4, s.size() + 1);
    PushByte(0);
    for (size_t i = s.size(); i-- > 0;) PushByte((uint8_t)s[i]);
    Push<uint32_t>((uint32_t)s.size());
    return (uint32_t)used_;
  }
  // a vector of offsets to objects written before
  uint32_t OffsetVector(const std::vector<uint32_t>& objs) {
    Align(4, 4 * objs.size());
    for (size_t i = objs.size(); i-- > 0;) PushOffset(objs[i]);
    Push<uint32_t>((uint32_t)objs.size());
    return (uint32_t)used_;
  }
  // a vector of structs of two int64 (FieldNode, Buffer)
  uint32_t PairVector(const std::vector<std::pair<int64_t, int64_t>>& v) {
    Align(4, 16 * v.size());
    Align(8, 16 * v.size());
    for (size_t i = v.size(); i-- > 0;) { Push<int64_t>(v[i].second); Push<int64_t>(v[i].first); }
    Push<uint32_t>((uint32_t)v.size());
    return (uint32_t)used_;
  }
  void StartTable() { fields_.clear(); table_start_ = used_; }
  template <typename T>
  void Scalar(int id, T v) { Push<T>(v); Note(id); }
  void Offset(int id, uint32_t obj) {
    if (!obj) return;
    PushOffset(obj);
    Note(id);
  }
  uint32_t EndTable() {
    Push<int32_t>(0);   // the offset to the vtable, patched below
    const size_t table = used_;
    const size_t nfields = fields_.size();
    for (size_t i = nfields; i-- > 0;) Push<uint16_t>((uint16_t)(fields_[i] ? table - fields_[i] : 0));
    Push<uint16_t>((uint16_t)(table - table_start_));
    Push<uint16_t>((uint16_t)(4 + 2 * nfields));
    Patch32(table, (uint32_t)(used_ - table));   // table address − vtable address
    return (uint32_t)table;
  }
  // the finished buffer: root offset first, length a multiple of 8
  std::vector<uint8_t> Finish(uint32_t root) {
    Align(8, 4);
    PushOffset(root);
    return std::vector<uint8_t>(rev_.rbegin(), rev_.rend());
  }

 private:
  void PushByte(uint8_t b) { rev_.push_back(b); used_++; }
  void PushOffset(uint32_t obj) {
    Align(4);
    Push<uint32_t>((uint32_t)(used_ + 4 - obj));
  }
  void Note(int id) {
    if ((size_t)id >= fields_.size()) fields_.resize((size_t)id + 1, 0);
    fields_[(size_t)id] = used_;
  }
  void Patch32(size_t pos, uint32_t v) {   // the 4 bytes whose position (from the end) is pos
    for (int i = 0; i < 4; i++) rev_[pos - 1 - (size_t)i] = (uint8_t)(v >> (8 * i));
  }
  std::vector<uint8_t> rev_;   // the buffer reversed: rev_[k] is the byte at position k + 1 from the end
  size_t used_ = 0, table_start_ = 0;
  std::vector<size_t> fields_;
};

// format/Message.fbs, format/Schema.fbs
enum { kHeaderSchema = 1, kHeaderDictionaryBatch = 2, kHeaderRecordBatch = 3 };
enum { kTypeInt = 2, kTypeFloatingPoint = 3, kTypeBinary = 4, kTypeUtf8 = 5, kTypeBool = 6, kTypeDate = 8, kTypeTime = 9, kTypeTimestamp = 10,
       kTypeDuration = 18, kTypeLargeBinary = 19, kTypeLargeUtf8 = 20 };
constexpr int16_t kMetadataV5 = 4;

int UnitOf(char c) { return c == 's' ? 0 : c == 'm' ? 1 : c == 'u' ? 2 : c == 'n' ? 3 : -1; }

bool IntBits(Type id, int* bits, bool* sgn) {
  switch (id) {
    case Type::INT8: *bits = 8; *sgn = true; return true;
    case Type::UINT8: *bits = 8; *sgn = false; return true;
    case Type::INT16: *bits = 16; *sgn = true; return true;
    case Type::UINT16: *bits = 16; *sgn = false; return true;
    case Type::INT32: *bits = 32; *sgn = true; return true;
    case Type::UINT32: *bits = 32; *sgn = false; return true;
    case Type::INT64: *bits = 64; *sgn = true; return true;
    case Type::UINT64: *bits = 64; *sgn = false; return true;
    default: return false;
  }
}
uint32_t IntTable(FbBuilder& fb, int bits, bool sgn) {
  fb.StartTable();
  fb.Scalar<int32_t>(0, bits);
  fb.Scalar<uint8_t>(1, sgn ? 1 : 0);
  return fb.EndTable();
}

// the Type union member of a field: false = a type this writer does not take
bool TypeTable(FbBuilder& fb, const FieldInfo& f, int* type_type, uint32_t* table) {
  auto empty = [&](int tt) { fb.StartTable(); *table = fb.EndTable(); *type_type = tt; return true; };
  auto unit_only = [&](int tt, int unit) {
    fb.StartTable();
    fb.Scalar<int16_t>(0, (int16_t)unit);
    *table = fb.EndTable();
    *type_type = tt;
    return true;
  };
  const std::string& l = f.logical;
  if (!l.empty()) {
    if (TemporalStorage(l) != f.type) return false;
    if (l == "tdD") return unit_only(kTypeDate, 0);
    if (l == "tdm") return unit_only(kTypeDate, 1);
    if (l[1] == 't') {
      fb.StartTable();
      fb.Scalar<int16_t>(0, (int16_t)UnitOf(l[2]));
      fb.Scalar<int32_t>(1, f.type->bit_width);
      *table = fb.EndTable();
      *type_type = kTypeTime;
      return true;
    }
    if (l[1] == 'D') return unit_only(kTypeDuration, UnitOf(l[2]));
    if (l[1] == 's') {
      const std::string tz = l.substr(4);
      const uint32_t tzs = tz.empty() ? 0 : fb.String(tz);
      fb.StartTable();
      fb.Scalar<int16_t>(0, (int16_t)UnitOf(l[2]));
      fb.Offset(1, tzs);
      *table = fb.EndTable();
      *type_type = kTypeTimestamp;
      return true;
    }
    return false;
  }
  int bits;
  bool sgn;
  if (IntBits(f.type->id, &bits, &sgn)) { *table = IntTable(fb, bits, sgn); *type_type = kTypeInt; return true; }
  switch (f.type->id) {
    case Type::FLOAT32: fb.StartTable(); fb.Scalar<int16_t>(0, 1); *table = fb.EndTable(); *type_type = kTypeFloatingPoint; return true;
    case Type::FLOAT64: fb.StartTable(); fb.Scalar<int16_t>(0, 2); *table = fb.EndTable(); *type_type = kTypeFloatingPoint; return true;
    case Type::BOOL: return empty(kTypeBool);
    case Type::STRING: return empty(kTypeUtf8);
    case Type::BINARY: return empty(kTypeBinary);
    case Type::LARGE_STRING: return empty(kTypeLargeUtf8);
    case Type::LARGE_BINARY: return empty(kTypeLargeBinary);
    default: return false;
  }
}

std::vector<uint8_t> FinishMessage(FbBuilder& fb, int header_type, uint32_t header, int64_t body_len) {
  fb.StartTable();
  fb.Scalar<int64_t>(3, body_len);
  fb.Offset(2, header);
  fb.Scalar<uint8_t>(1, (uint8_t)header_type);
  fb.Scalar<int16_t>(0, kMetadataV5);
  return fb.Finish(fb.EndTable());
}

// RecordBatch { length; nodes; buffers; compression }
uint32_t RecordBatchTable(FbBuilder& fb, int64_t rows, const std::vector<std::pair<int64_t, int64_t>>& nodes,
                          const std::vector<std::pair<int64_t, int64_t>>& buffers, bool lz4) {
  uint32_t comp = 0;
  if (lz4) {   // BodyCompression { codec: LZ4_FRAME (0); method: BUFFER (0) }
    fb.StartTable();
    fb.Scalar<int8_t>(0, 0);
    fb.Scalar<int8_t>(1, 0);
    comp = fb.EndTable();
  }
  const uint32_t bv = fb.PairVector(buffers);
  const uint32_t nv = fb.PairVector(nodes);
  fb.StartTable();
  fb.Scalar<int64_t>(0, rows);
  fb.Offset(1, nv);
  fb.Offset(2, bv);
  fb.Offset(3, comp);
  return fb.EndTable();
}

void AppendFramed(std::vector<uint8_t>* out, const std::vector<uint8_t>& meta) {   // continuation, length, metadata (a multiple of 8)
  const uint32_t cont = 0xFFFFFFFFu, len = (uint32_t)meta.size();
  const uint8_t* c = (const uint8_t*)&cont;
  const uint8_t* l = (const uint8_t*)&len;
  out->insert(out->end(), c, c + 4);
  out->insert(out->end(), l, l + 4);
  out->insert(out->end(), meta.begin(), meta.end());
}

// the identical device buffers, cut the same way (the writer keeps the dictionary it wrote last alive, so an address cannot have
// been given to another array in between)
bool SameBuffers(const ArrayData& a, const ArrayData& b) {
  for (int i = 0; i < 3; i++)
    if ((a.buffers[i] ? a.buffers[i]->dptr : nullptr) != (b.buffers[i] ? b.buffers[i]->dptr : nullptr)) return false;
  return a.offset == b.offset && a.length == b.length && a.type == b.type;
}

constexpr int64_t kPiece = 65536;   // bytes per compressed block, and per row of the pack where plain bytes move

}  // namespace

StreamWriter::StreamWriter(Session* s, bool lz4) : s_(s), lz4_(lz4) {}

// what one column is on the wire, from the array itself
Status StreamWriter::Describe(const std::string& name, const ArrayData& a, int64_t next_dict_id, FieldInfo* out) const {
  out->name = name;
  out->nullable = true;
  if (a.on_host) return Invalid("column '" + name + "' lives in host memory; the writer takes device arrays");
  if (!a.type) return Invalid("column '" + name + "' has no type");
  if (a.type->id == Type::DICTIONARY) {
    if (!a.dictionary || !a.dict_value_type) return Invalid("column '" + name + "' is dictionary-encoded without a dictionary");
    out->type = a.dict_value_type;
    out->logical = a.dictionary->logical;
    out->dict_id = next_dict_id;
    out->index_type = a.dict_index_type ? a.dict_index_type : GetDataType(Type::INT32);
    if (a.dictionary->type->id == Type::DICTIONARY) return NotImpl("column '" + name + "': a dictionary of dictionary-encoded values");
  } else {
    out->type = a.type;
    out->logical = a.logical;
  }
  FbBuilder probe;
  int tt;
  uint32_t table;
  if (!TypeTable(probe, *out, &tt, &table))
    return NotImpl("column '" + name + "': type " + (out->logical.empty() ? std::string(out->type->name) : out->logical) + " is not written");
  return Status::OK();
}

Status StreamWriter::WriteSchema() {
  FbBuilder fb;
  std::vector<uint32_t> fields;
  for (const FieldInfo& f : fields_) {
    int tt = 0;
    uint32_t type = 0, dict = 0;
    TypeTable(fb, f, &tt, &type);
    if (f.dict_id >= 0) {   // DictionaryEncoding { id; indexType; isOrdered; dictionaryKind }
      int bits = 32;
      bool sgn = true;
      IntBits(f.index_type->id, &bits, &sgn);
      const uint32_t it = IntTable(fb, bits, sgn);
      fb.StartTable();
      fb.Scalar<int64_t>(0, f.dict_id);
      fb.Offset(1, it);
      fb.Scalar<uint8_t>(2, 0);
      dict = fb.EndTable();
    }
    const uint32_t children = fb.OffsetVector({});
    const uint32_t name = fb.String(f.name);
    fb.StartTable();
    fb.Offset(0, name);
    fb.Scalar<uint8_t>(1, 1);
    fb.Scalar<uint8_t>(2, (uint8_t)tt);
    fb.Offset(3, type);
    fb.Offset(4, dict);
    fb.Offset(5, children);
    fields.push_back(fb.EndTable());
  }
  const uint32_t fv = fb.OffsetVector(fields);
  fb.StartTable();
  fb.Scalar<int16_t>(0, 0);   // little-endian
  fb.Offset(1, fv);
  const uint32_t schema = fb.EndTable();
  AppendFramed(&out_, FinishMessage(fb, kHeaderSchema, schema, 0));
  return Status::OK();
}

// One column of one message: the plain bytes of its buffers, normalised into the staging allocation.
struct StreamWriter::Piece {
  int64_t at = 0, len = 0;   // in the staging allocation
};
struct StreamWriter::Column {
  const ArrayData* a = nullptr;
  const DataType* storage = nullptr;   // what the data buffer holds on the wire (a dictionary column: the index type)
  bool indices = false;                // … converted from the device's int32
  int64_t nulls = 0, first = 0, last = 0;
  int nbuf = 0;
  Piece bufs[3];
};
struct StreamWriter::Message {
  int header = 0;
  int64_t dict_id = -1;
  int64_t rows = 0;
  std::vector<Column> cols;
};

Status StreamWriter::Write(const std::vector<std::string>& names, const std::vector<ArrayDataPtr>& columns) {
  if (closed_) return Invalid("the stream was finished");
  if (names.size() != columns.size()) return Invalid("as many names as columns");
  // ---- the schema: fixed by the first batch, checked on the others ------------------------------------------------------------
  std::vector<FieldInfo> fields;
  int64_t next_id = 0;
  for (size_t i = 0; i < columns.size(); i++) {
    if (!columns[i]) return Invalid("column '" + names[i] + "' is null");
    FieldInfo f;
    AHC_RETURN_NOT_OK(Describe(names[i], *columns[i], next_id, &f));
    if (f.dict_id >= 0) next_id++;
    fields.push_back(std::move(f));
  }
  for (size_t i = 0; i < columns.size(); i++)
    if (columns[i]->length != columns[0]->length)
      return Invalid("column '" + names[i] + "' has " + std::to_string(columns[i]->length) + " rows, column '" + names[0] + "' " + std::to_string(columns[0]->length));
  if (!have_schema_) {
    fields_ = fields;
    AHC_RETURN_NOT_OK(WriteSchema());
    have_schema_ = true;
  } else {
    if (fields.size() != fields_.size()) return Invalid("the batch has " + std::to_string(fields.size()) + " columns, the schema " + std::to_string(fields_.size()));
    for (size_t i = 0; i < fields.size(); i++) {
      const FieldInfo &a = fields[i], &b = fields_[i];
      if (a.name != b.name) return Invalid("column " + std::to_string(i) + " is named '" + a.name + "', the schema's is '" + b.name + "'");
      if (a.type != b.type || a.logical != b.logical || a.dict_id != b.dict_id || a.index_type != b.index_type)
        return Invalid("column '" + a.name + "' does not have the type the first batch fixed for it");
    }
  }
  const int64_t rows = columns.empty() ? 0 : columns[0]->length;

  // ---- the messages of this call: dictionaries first ----------------------------------------------------------------------------
  std::vector<Message> msgs;
  std::vector<std::pair<int64_t, ArrayDataPtr>> new_dicts;
  for (size_t i = 0; i < columns.size(); i++) {
    if (fields_[i].dict_id < 0) continue;
    const ArrayData& d = *columns[i]->dictionary;
    if (d.on_host) return Invalid("column '" + names[i] + "': its dictionary lives in host memory");
    auto it = written_dicts_.find(fields_[i].dict_id);
    if (it != written_dicts_.end() && SameBuffers(*it->second, d)) continue;
    Message m;
    m.header = kHeaderDictionaryBatch;
    m.dict_id = fields_[i].dict_id;
    m.rows = d.length;
    Column c;
    c.a = &d;
    c.storage = d.type;
    m.cols.push_back(c);
    msgs.push_back(std::move(m));
    new_dicts.push_back({fields_[i].dict_id, columns[i]->dictionary});
  }
  {
    Message m;
    m.header = kHeaderRecordBatch;
    m.rows = rows;
    for (size_t i = 0; i < columns.size(); i++) {
      Column c;
      c.a = columns[i].get();
      c.indices = fields_[i].dict_id >= 0;
      c.storage = c.indices ? fields_[i].index_type : fields_[i].type;
      m.cols.push_back(c);
    }
    msgs.push_back(std::move(m));
  }

  // ---- what every buffer holds: null counts, and the referenced range of var-length data -----------------------------------------
  // (a column whose null count is unknown costs one popcount with its own wait; the offsets' ends of all columns share one)
  ah_ctx* ctx = s_->ctx();
  std::vector<uint8_t> ends;
  for (Message& m : msgs)
    for (Column& c : m.cols) {
      const ArrayData& a = *c.a;
      c.nulls = 0;
      if (a.length > 0 && a.buffers[0] && a.null_count != 0) {
        if (a.null_count > 0) {
          c.nulls = a.null_count;
        } else {
          int64_t set = 0;
          AHC_RETURN_NOT_OK(s_->FromStatus(ah_count_set_bits(ctx, (const uint8_t*)a.buffers[0]->dptr, a.offset, a.length, &set)));
          c.nulls = a.length - set;
        }
      }
      if (IsBaseBinary(c.storage->id) && a.length > 0) {
        if (!a.buffers[1]) return Invalid("a var-length column without offsets");
        ends.resize(ends.size() + 16, 0);
      }
    }
  {
    size_t at = 0;
    for (Message& m : msgs)
      for (Column& c : m.cols) {
        const ArrayData& a = *c.a;
        if (!IsBaseBinary(c.storage->id) || a.length == 0) continue;
        const int w = c.storage->bit_width / 8;
        const uint8_t* o = (const uint8_t*)a.buffers[1]->dptr;
        AHC_RETURN_NOT_OK(s_->FromStatus(ah_download_async(ctx, &ends[at], o + a.offset * w, (size_t)w)));
        AHC_RETURN_NOT_OK(s_->FromStatus(ah_download_async(ctx, &ends[at + 8], o + (a.offset + a.length) * w, (size_t)w)));
        at += 16;
      }
    if (at) AHC_RETURN_NOT_OK(s_->FromStatus(ah_sync(ctx)));
    at = 0;
    for (Message& m : msgs)
      for (Column& c : m.cols) {
        const ArrayData& a = *c.a;
        if (!IsBaseBinary(c.storage->id) || a.length == 0) continue;
        if (c.storage->bit_width == 32) { int32_t x, y; std::memcpy(&x, &ends[at], 4); std::memcpy(&y, &ends[at + 8], 4); c.first = x; c.last = y; }
        else { std::memcpy(&c.first, &ends[at], 8); std::memcpy(&c.last, &ends[at + 8], 8); }
        at += 16;
        if (c.first < 0 || c.last < c.first || c.last > (a.buffers[2] ? a.buffers[2]->size : 0))
          return Invalid("a var-length column whose offsets leave its data buffer");
      }
  }

  // ---- the staging allocation: every buffer's plain bytes, each piece on a multiple of 64 -----------------------------------------
  int64_t staged = 0;
  auto place = [&](Piece* p, int64_t len) { p->at = staged; p->len = len; staged += (len + 63) & ~(int64_t)63; };
  for (Message& m : msgs)
    for (Column& c : m.cols) {
      const ArrayData& a = *c.a;
      const int64_t n = a.length;
      place(&c.bufs[0], c.nulls > 0 ? (n + 7) / 8 : 0);
      if (IsBaseBinary(c.storage->id)) {
        c.nbuf = 3;
        place(&c.bufs[1], n > 0 ? (n + 1) * (c.storage->bit_width / 8) : 0);
        place(&c.bufs[2], c.last - c.first);
      } else {
        c.nbuf = 2;
        place(&c.bufs[1], c.storage->bit_width == 1 ? (n + 7) / 8 : n * (c.storage->bit_width / 8));
      }
    }
  BufferPtr stage;
  AHC_RETURN_NOT_OK(s_->Allocate(staged > 0 ? staged : 64, &stage, /*zero_all=*/false));
  uint8_t* sp = (uint8_t*)stage->dptr;
  auto bits_to = [&](const Piece& p, const uint8_t* src, int64_t off, int64_t n) -> Status {   // bits [off, off + n) → bit 0 on, the rest of the last byte zero
    AHC_RETURN_NOT_OK(s_->FromStatus(ah_memset_async(ctx, sp + p.at, 0, (size_t)p.len)));
    return s_->FromStatus(ah_copy_bitmap(ctx, src, off, n, sp + p.at, 0, 0));
  };
  for (Message& m : msgs)
    for (Column& c : m.cols) {
      const ArrayData& a = *c.a;
      const int64_t n = a.length;
      if (c.bufs[0].len > 0) AHC_RETURN_NOT_OK(bits_to(c.bufs[0], (const uint8_t*)a.buffers[0]->dptr, a.offset, n));
      if (n == 0) continue;
      if (!a.buffers[1]) return Invalid("a column without a data buffer");
      const uint8_t* b1 = (const uint8_t*)a.buffers[1]->dptr;
      if (IsBaseBinary(c.storage->id)) {
        const int w = c.storage->bit_width / 8;
        const int64_t neg = -c.first;
        const int32_t neg32 = (int32_t)neg;
        AHC_RETURN_NOT_OK(s_->FromStatus(ah_arithmetic_arr_scalar(ctx, w == 4 ? AH_INT32 : AH_INT64, AH_OP_ADD, b1 + a.offset * w,
                                                                  w == 4 ? (const void*)&neg32 : (const void*)&neg, sp + c.bufs[1].at, n + 1)));
        if (c.bufs[2].len > 0)
          AHC_RETURN_NOT_OK(s_->FromStatus(ah_copy_async(ctx, sp + c.bufs[2].at, (const uint8_t*)a.buffers[2]->dptr + c.first, (size_t)c.bufs[2].len)));
      } else if (c.storage->bit_width == 1) {
        AHC_RETURN_NOT_OK(bits_to(c.bufs[1], b1, a.offset, n));
      } else if (c.indices && c.storage->id != Type::INT32) {   // the device's int32 indices → the producer's index type
        AHC_RETURN_NOT_OK(s_->FromStatus(ah_cast_numeric(ctx, AH_INT32, (int)c.storage->id, b1 + a.offset * 4, nullptr, 0, n, 1, 1, sp + c.bufs[1].at)));
      } else {
        const int w = c.indices ? 4 : c.storage->bit_width / 8;
        AHC_RETURN_NOT_OK(s_->FromStatus(ah_copy_async(ctx, sp + c.bufs[1].at, b1 + a.offset * w, (size_t)c.bufs[1].len)));
      }
    }

  // ---- compression: every 64 KiB piece of every buffer, one launch; slot i lies where block i lies in the staging layout ------------
  struct Span { size_t first_block = 0, nblocks = 0; };
  std::vector<Span> spans;
  std::vector<int64_t> table;
  std::vector<int32_t> sizes;
  std::vector<uint8_t> stored;
  BufferPtr comp;
  if (lz4_) {
    for (Message& m : msgs)
      for (Column& c : m.cols)
        for (int b = 0; b < c.nbuf; b++) {
          Span sp_{table.size() / 3, 0};
          for (int64_t o = 0; o < c.bufs[b].len; o += kPiece) {
            const int64_t len = c.bufs[b].len - o < kPiece ? c.bufs[b].len - o : kPiece;
            table.insert(table.end(), {c.bufs[b].at + o, len, c.bufs[b].at + o});
            sp_.nblocks++;
          }
          spans.push_back(sp_);
        }
    const int64_t nblocks = (int64_t)table.size() / 3;
    sizes.resize((size_t)nblocks);
    stored.resize((size_t)nblocks);
    if (nblocks > 0) {
      AHC_RETURN_NOT_OK(s_->Allocate(staged, &comp, /*zero_all=*/false));
      AHC_RETURN_NOT_OK(s_->FromStatus(ah_lz4_compress_blocks(ctx, sp, staged, (uint8_t*)comp->dptr, staged, table.data(), nblocks, sizes.data(), stored.data())));
    }
  }

  // ---- the layout of everything this call appends, and the rows that put it together --------------------------------------------------
  std::vector<uint8_t> lits;
  std::vector<int64_t> rows_tab;
  int64_t at = 0;   // position in what this call appends
  auto lit_row = [&](const uint8_t* p, int64_t n) {
    if (n == 0) return;
    rows_tab.insert(rows_tab.end(), {(int64_t)lits.size(), n, at, 2});
    lits.insert(lits.end(), p, p + n);
    at += n;
  };
  auto plain_rows = [&](int64_t src, int64_t n) {
    for (int64_t o = 0; o < n; o += kPiece) {
      const int64_t len = n - o < kPiece ? n - o : kPiece;
      rows_tab.insert(rows_tab.end(), {src + o, len, at, 1});
      at += len;
    }
  };
  static const uint8_t kZeros[8] = {0};
  uint8_t frame_header[7];
  lz4::FrameHeader(frame_header);
  size_t span_i = 0;
  int64_t raw_total = 0, written_total = 0, n_compressed = 0, n_raw = 0;
  struct Layout { std::vector<std::pair<int64_t, int64_t>> nodes, buffers; int64_t body_len = 0; };
  // per message: the buffers' places inside the body first (the metadata names them), then the metadata's row, then the body's rows
  for (Message& m : msgs) {
    Layout lay;
    int64_t body = 0;
    struct BufPlan { bool framed = false, raw = false; std::vector<int64_t> bsizes; Span span; Piece piece; int64_t wire_len = 0; };
    std::vector<BufPlan> plans;
    for (Column& c : m.cols) {
      lay.nodes.push_back({c.a->length, c.nulls});
      for (int b = 0; b < c.nbuf; b++) {
        BufPlan p;
        p.piece = c.bufs[b];
        if (lz4_) p.span = spans[span_i++];
        const int64_t len = p.piece.len;
        if (len == 0) {
          p.wire_len = 0;
        } else if (lz4_) {
          for (size_t k = 0; k < p.span.nblocks; k++) p.bsizes.push_back(sizes[p.span.first_block + k]);
          const int64_t framed = lz4::FramedBytes(p.bsizes);
          if (framed - lz4::kFramePrefix < len) { p.framed = true; p.wire_len = framed; n_compressed++; }
          else { p.raw = true; p.wire_len = lz4::kFramePrefix + len; n_raw++; }
        } else {
          p.wire_len = len;
        }
        lay.buffers.push_back({body, p.wire_len});
        body += lz4::Pad8(p.wire_len);
        raw_total += len;
        written_total += lz4::Pad8(p.wire_len);
        plans.push_back(std::move(p));
      }
    }
    lay.body_len = body;
    // the metadata of this message
    FbBuilder fb;
    uint32_t header = RecordBatchTable(fb, m.rows, lay.nodes, lay.buffers, lz4_);
    if (m.header == kHeaderDictionaryBatch) {   // DictionaryBatch { id; data; isDelta }
      fb.StartTable();
      fb.Scalar<int64_t>(0, m.dict_id);
      fb.Offset(1, header);
      fb.Scalar<uint8_t>(2, 0);
      header = fb.EndTable();
    }
    std::vector<uint8_t> framed_meta;
    AppendFramed(&framed_meta, FinishMessage(fb, m.header, header, body));
    lit_row(framed_meta.data(), (int64_t)framed_meta.size());
    // the body
    for (const BufPlan& p : plans) {
      const int64_t start = at;
      if (p.wire_len == 0) continue;
      if (p.framed) {
        uint8_t head[15];
        const int64_t ulen = p.piece.len;
        std::memcpy(head, &ulen, 8);
        std::memcpy(head + 8, frame_header, 7);
        lit_row(head, 15);
        for (size_t k = 0; k < p.span.nblocks; k++) {
          const size_t blk = p.span.first_block + k;
          const uint64_t word = (uint64_t)(uint32_t)sizes[blk] | (stored[blk] ? 0x80000000u : 0u);
          rows_tab.insert(rows_tab.end(), {table[3 * blk + 2], (int64_t)sizes[blk], at + 4, (int64_t)((word << 32) | 0x100u)});
          at += 4 + sizes[blk];
        }
        uint8_t tail[4 + 8] = {0};
        lit_row(tail, 4 + (lz4::Pad8(p.wire_len) - p.wire_len));
      } else {
        if (p.raw) {
          const int64_t minus_one = -1;
          lit_row((const uint8_t*)&minus_one, 8);
        }
        plain_rows(p.piece.at, p.piece.len);
        lit_row(kZeros, lz4::Pad8(p.wire_len) - p.wire_len);
      }
      if (at - start != lz4::Pad8(p.wire_len)) return Invalid("internal: a buffer's layout does not add up");
    }
  }

  // ---- one launch puts it together, one copy brings it down ----------------------------------------------------------------------------
  BufferPtr packed;
  AHC_RETURN_NOT_OK(s_->Allocate(at, &packed, /*zero_all=*/false));
  AHC_RETURN_NOT_OK(s_->FromStatus(ah_ipc_pack_body(ctx, comp ? (const uint8_t*)comp->dptr : nullptr, comp ? staged : 0, sp, staged, lits.data(), (int64_t)lits.size(),
                                                    rows_tab.data(), (int64_t)rows_tab.size() / 4, (uint8_t*)packed->dptr, at)));
  const size_t old = out_.size();
  out_.resize(old + (size_t)at);
  Status done = s_->FromStatus(ah_download_async(ctx, out_.data() + old, packed->dptr, (size_t)at));
  const Status waited = s_->FromStatus(ah_sync(ctx));   // on both paths: nothing in flight writes into out_ afterwards
  if (done.ok()) done = waited;
  if (!done.ok()) { out_.resize(old); return done; }   // a Write that fails appends nothing
  for (auto& nd : new_dicts) written_dicts_[nd.first] = nd.second;
  stats_[0] += raw_total; stats_[1] += written_total; stats_[2] += n_compressed; stats_[3] += n_raw;
  return Status::OK();
}

Status StreamWriter::Close() {
  if (closed_) return Status::OK();
  if (!have_schema_) return Invalid("a stream needs a schema: no batch was written");
  static const uint8_t eos[8] = {0xFF, 0xFF, 0xFF, 0xFF, 0, 0, 0, 0};
  out_.insert(out_.end(), eos, eos + 8);
  closed_ = true;
  return Status::OK();
}

}  // namespace ipc
}  // namespace arrowhip

// the C API (include/arrowhip_compute.h); defined here so that the rest of the host layer links without the writer
using namespace arrowhip;

// ---- HBM-resident record batches → an Arrow IPC stream (ipc.NewWriter / Writer.Write / Close, arrow/ipc/writer.go:85-260) ----
struct ahc_ipc_writer {
  ahc_session* s;
  std::unique_ptr<ipc::StreamWriter> w;
};

// options: "compression=lz4" (also for NULL / "") or "compression=none"
extern "C" __attribute__((visibility("default"))) int ahc_ipc_writer_open(ahc_session* s, const char* options, ahc_ipc_writer** out) {
  *out = nullptr;
  const std::string o = options ? options : "";
  bool lz4 = true;
  if (o == "compression=none") lz4 = false;
  else if (!o.empty() && o != "compression=lz4")
    return ahc_internal_fail(s, Status::Make(StatusCode::Invalid, "arrow/ipc: writer options '" + o + "': expected compression=lz4 or compression=none"));
  *out = new ahc_ipc_writer{s, std::unique_ptr<ipc::StreamWriter>(new ipc::StreamWriter(ahc_internal_session(s), lz4))};
  return 0;
}
extern "C" __attribute__((visibility("default"))) int ahc_ipc_write_batch(ahc_ipc_writer* w, int ncols, const char* const* names, ahc_datum** columns) {
  if (ncols < 0 || (ncols > 0 && (!names || !columns))) return ahc_internal_fail(w->s, Status::Make(StatusCode::Invalid, "arrow/ipc: write_batch without columns"));
  std::vector<std::string> ns;
  std::vector<ArrayDataPtr> cols;
  for (int i = 0; i < ncols; i++) {
    const std::string name = names[i] ? names[i] : "";
    if (!columns[i]) return ahc_internal_fail(w->s, Status::Make(StatusCode::Invalid, "arrow/ipc: column '" + name + "' is null"));
    const compute::Datum& d = *ahc_internal_datum(columns[i]);
    if (d.kind == compute::DatumKind::Chunked)
      return ahc_internal_fail(w->s, Status::Make(StatusCode::Invalid, "arrow/ipc: column '" + name + "' is chunked: write it chunk by chunk, one batch per chunk"));
    if (d.kind != compute::DatumKind::Array || !d.array)
      return ahc_internal_fail(w->s, Status::Make(StatusCode::Invalid, "arrow/ipc: column '" + name + "' is not an array datum (a scalar has no rows to write: write chunk by chunk, arrays only)"));
    ns.push_back(name);
    cols.push_back(d.array);
  }
  Status st = w->w->Write(ns, cols);
  return st.ok() ? 0 : ahc_internal_fail(w->s, st);
}
// the end-of-stream marker; *bytes stays valid until ahc_ipc_writer_close
extern "C" __attribute__((visibility("default"))) int ahc_ipc_writer_finish(ahc_ipc_writer* w, const uint8_t** bytes, int64_t* len) {
  Status st = w->w->Close();
  if (!st.ok()) return ahc_internal_fail(w->s, st);
  *bytes = w->w->bytes().data();
  *len = (int64_t)w->w->bytes().size();
  return 0;
}
extern "C" __attribute__((visibility("default"))) void ahc_ipc_writer_stats(ahc_ipc_writer* w, int64_t out[4]) { w->w->stats(out); }
extern "C" __attribute__((visibility("default"))) void ahc_ipc_writer_close(ahc_ipc_writer* w) { delete w; }
