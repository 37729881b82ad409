/* Host glue, not part of the C ABI: hands the UTF-8 bytes of a Python list of str to libamdretrieval WITHOUT copying
 * them.  amdr_tokenizer_encode_ptrs (include/amdretrieval.h) takes plain `const char*` / length arrays; for a caller that
 * holds Python strings the cheapest way to those is CPython's own cached UTF-8 view of each object
 * (PyUnicode_AsUTF8AndSize: for an ASCII string the pointer INTO the object, no allocation) — "\0".join(qs).encode()
 * touches and copies every string and was 70 % of a 9 344-query tokeniser call.  The list must stay alive while the
 * pointers are in use (the caller holds it across the native call).
 *
 *   utf8_views(seq, ptrs_addr, lens_addr[, wide_addr]) -> total bytes
 *     seq: list / tuple of str (None counts as ""), ptrs_addr / lens_addr: addresses of int64 arrays of len(seq) entries;
 *     wide_addr (optional): address of a uint8 array of len(seq) entries, set to 1 where the string's storage kind
 *     admits code points >= U+4E00 (UCS-2 / UCS-4: it MAY hold a Han character — an O(1) read of the object's kind,
 *     no scan) and 0 where it cannot (ASCII / Latin-1: certainly no Han character)
 */
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <stdint.h>

static PyObject* utf8_views(PyObject* self, PyObject* args) {
  PyObject* seq;
  unsigned long long pa, la, wa = 0;
  if (!PyArg_ParseTuple(args, "OKK|K", &seq, &pa, &la, &wa)) return NULL;
  PyObject* fast = PySequence_Fast(seq, "utf8_views: a sequence of str is required");
  if (!fast) return NULL;
  const Py_ssize_t n = PySequence_Fast_GET_SIZE(fast);
  PyObject** items = PySequence_Fast_ITEMS(fast);
  int64_t* ptrs = (int64_t*)(uintptr_t)pa;
  int64_t* lens = (int64_t*)(uintptr_t)la;
  uint8_t* wide = (uint8_t*)(uintptr_t)wa;
  int64_t total = 0;
  static const char kEmpty[1] = {0};
  for (Py_ssize_t i = 0; i < n; ++i) {
    PyObject* o = items[i];
    if (o == Py_None) {
      ptrs[i] = (int64_t)(uintptr_t)kEmpty;
      lens[i] = 0;
      if (wide) wide[i] = 0;
      continue;
    }
    if (!PyUnicode_Check(o)) {
      Py_DECREF(fast);
      PyErr_Format(PyExc_TypeError, "utf8_views: item %zd is not a str", i);
      return NULL;
    }
    Py_ssize_t len = 0;
    const char* p = PyUnicode_AsUTF8AndSize(o, &len);
    if (!p) {
      Py_DECREF(fast);
      return NULL;
    }
    ptrs[i] = (int64_t)(uintptr_t)p;
    lens[i] = (int64_t)len;
    if (wide) wide[i] = PyUnicode_MAX_CHAR_VALUE(o) >= 0x4E00 ? 1 : 0;
    total += (int64_t)len;
  }
  Py_DECREF(fast);
  return PyLong_FromLongLong((long long)total);
}

static PyMethodDef kMethods[] = {{"utf8_views", utf8_views, METH_VARARGS, "UTF-8 pointers and sizes of a list of str"},
                                 {NULL, NULL, 0, NULL}};
static struct PyModuleDef kModule = {PyModuleDef_HEAD_INIT, "_amdr_pystrings", NULL, -1, kMethods, NULL, NULL, NULL, NULL};
PyMODINIT_FUNC PyInit__amdr_pystrings(void) { return PyModule_Create(&kModule); }
